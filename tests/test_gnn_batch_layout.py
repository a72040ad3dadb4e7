"""CPU: the layout of mlamg.gnn.GraphBatch — the block-diagonal stack FullAggNet.forward_batch runs
on — is Graph's layout of scipy.sparse.block_diag of the same matrices, field for field, with
x = 1/n_g per graph and cumulative segment pointers; a matrix without canonical format is refused
by index. Graph and GraphBatch share one builder of these fields, so it is also pinned on its own,
to arrays written out by hand for a small matrix in non-canonical stored order. No GPU:
device="cpu"."""
import numpy as np
import pytest
import scipy.sparse as sp


def _As():
    from mlamg import problems
    return [problems.poisson_1d(1), problems.poisson_2d_5pt(5), problems.poisson_2d_5pt(7, 9),
            problems.jump_2d(12, problems.voronoi_jumps(np.random.RandomState(0)))]


def _hand_csr():
    """4 x 4, stored order kept: row 0 unsorted (columns 2, 0), row 1 a duplicate entry (1, 1),
    row 2 empty, row 3 one entry; (0, 2) and (3, 0) have no transposed partner."""
    A = sp.csr_matrix((np.array([-1.0, 2.0, 0.5, -0.25, 3.0]), np.array([2, 0, 1, 1, 0]),
                       np.array([0, 2, 4, 4, 5])), shape=(4, 4))
    assert not A.has_canonical_format and A.indices.tolist() == [2, 0, 1, 1, 0]
    return A


def test_graph_fields_by_definition():
    """The one builder behind Graph and GraphBatch against arrays written out by hand: edges in
    stored order, teid = the stable sort of the edges by target, x = float32(1 / 4)."""
    import torch
    from mlamg import gnn
    A = _hand_csr()
    g = gnn.Graph(A, device="cpu")
    assert (g.nb, g.n, g.E, g.fe) == (1, 4, 5, 1)
    want = dict(crow=np.array([0, 2, 4, 4, 5], dtype=np.int32),
                src=np.array([0, 0, 1, 1, 3], dtype=np.int32),
                tgt=np.array([2, 0, 1, 1, 0], dtype=np.int32),
                tptr=np.array([0, 2, 4, 5, 5], dtype=np.int32),
                teid=np.array([1, 4, 2, 3, 0], dtype=np.int32),
                edge_attr=np.array([[1.0], [2.0], [0.5], [0.25], [3.0]], dtype=np.float32),
                x=np.full((4, 1), np.float32(1.0 / 4), dtype=np.float32))
    for name, ref in want.items():
        mine = getattr(g, name)
        assert mine.dtype == torch.as_tensor(ref).dtype and tuple(mine.shape) == ref.shape, name
        assert torch.equal(mine, torch.as_tensor(ref)), name
    assert g.seg.host.dtype == np.int64 and g.seg.host.tolist() == [0, 4]
    assert g.eseg.host.dtype == np.int64 and g.eseg.host.tolist() == [0, 5]
    with pytest.raises(ValueError, match=r"matrix 0\b"):
        gnn.GraphBatch([A], device="cpu")


def test_graph_agg_is_with_clusters_of_argmax():
    """Row 2 of Agg is all zero: argmax gives 0 there, the -1 -> 0 rule of with_clusters."""
    import torch
    from mlamg import gnn
    A = _hand_csr()
    Agg = sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0], [0.0, 0.0], [0.0, 1.0]]))
    ga = gnn.Graph(A, agg=Agg, device="cpu")
    col = torch.as_tensor(np.asarray(Agg.argmax(axis=1)).ravel())
    assert col.tolist() == [1, 0, 0, 1]
    plain = gnn.Graph(A, device="cpu")
    assert ga.fe == 2 and ga.edge_attr.dtype == torch.float32
    assert torch.equal(ga.edge_attr, plain.with_clusters(col).edge_attr)
    assert torch.equal(ga.edge_attr, plain.with_clusters(torch.tensor([1, 0, -1, 1])).edge_attr)
    # edges (0, 2), (0, 0), (1, 1), (1, 1), (3, 0): only the first joins two aggregates
    assert ga.edge_attr.tolist() == [[1.0, 1.0], [2.0, 0.0], [0.5, 0.0], [0.25, 0.0], [3.0, 0.0]]
    for name in ("crow", "src", "tgt", "tptr", "teid", "x"):
        assert torch.equal(getattr(ga, name), getattr(plain, name)), name


def test_layout_is_graph_of_block_diag():
    import torch
    from mlamg import gnn
    As = _As()
    b = gnn.GraphBatch(As, device="cpu")
    g = gnn.Graph(sp.block_diag(As).tocsr(), device="cpu")
    assert (b.n, b.E, b.fe, b.nb) == (g.n, g.E, g.fe, len(As))
    for name in ("crow", "src", "tgt", "tptr", "teid", "edge_attr", "edge_index"):
        mine, ref = getattr(b, name), getattr(g, name)
        assert mine.dtype == ref.dtype and mine.shape == ref.shape, name
        assert torch.equal(mine, ref), name
    assert b.x.dtype == torch.float32 and b.x.shape == (b.n, 1)


def test_x_and_segment_pointers():
    import torch
    from mlamg import gnn
    As = _As()
    b = gnn.GraphBatch(As, device="cpu")
    sizes = [A.shape[0] for A in As]
    nnzs = [A.nnz for A in As]
    assert b.seg.host.dtype == np.int64 and b.eseg.host.dtype == np.int64
    assert b.seg.host.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert b.eseg.host.tolist() == np.concatenate([[0], np.cumsum(nnzs)]).tolist()
    assert torch.equal(b.seg.dev, torch.as_tensor(b.seg.host))
    assert torch.equal(b.eseg.dev, torch.as_tensor(b.eseg.host))
    for g, n in enumerate(sizes):
        a = int(b.seg.host[g])
        # Graph's own constant: float32(1 / n)
        assert torch.equal(b.x[a:a + n], gnn.Graph(As[g], device="cpu").x), g
        assert b.node_gid[a:a + n].tolist() == [g] * n
    # k_g = ceil(alpha n_g), the rule of forward()
    for alpha in (0.02, 0.1, 0.3, 1.0):
        ks = [int(np.ceil(alpha * n)) for n in sizes]
        assert b.k_ptr(alpha).host.tolist() == np.concatenate([[0], np.cumsum(ks)]).tolist()


def test_with_clusters_matches_graph():
    import torch
    from mlamg import gnn
    As = _As()
    b = gnn.GraphBatch(As, device="cpu")
    g = gnn.Graph(sp.block_diag(As).tocsr(), device="cpu")
    col = torch.as_tensor((np.arange(b.n) // 3).astype(np.int32))
    col[5] = -1
    bc, gc = b.with_clusters(col), g.with_clusters(col)
    assert bc.fe == 2 and torch.equal(bc.edge_attr, gc.edge_attr)
    assert b.fe == 1 and b.edge_attr.shape == (b.E, 1)  # the batch itself is unchanged
    assert bc.crow is b.crow and bc.seg is b.seg


def test_non_canonical_matrix_is_refused_by_index():
    from mlamg import gnn, problems
    A = problems.poisson_2d_5pt(4)
    unsorted = sp.csr_matrix((A.data[::-1].copy(), A.indices[::-1].copy(),
                              A.indptr[-1] - A.indptr[::-1]), shape=A.shape)
    assert not unsorted.has_canonical_format
    dup = sp.csr_matrix((np.ones(3), np.array([0, 0, 1]), np.array([0, 2, 3])), shape=(2, 2))
    assert not dup.has_canonical_format
    for bad in (unsorted, dup):
        with pytest.raises(ValueError, match=r"matrix 2\b"):
            gnn.GraphBatch([A, A, bad, A], device="cpu")
    with pytest.raises(ValueError):
        gnn.GraphBatch([], device="cpu")
