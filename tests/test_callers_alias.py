"""CPU: the reference's callers resolve every hot-path name through mlamg.compat.install()
alone — with pyamg and torch_sparse absent. No GPU calls.

* The alias table: ns.lib.{multigrid, graph, sparse, sparse_tensor} and pyamg.{aggregation,
  graph, strength, relaxation.relaxation} resolve to this package, parents bound as attributes.
* ns.lib.sparse_tensor mirror (ns/lib/sparse_tensor.py:9-59) on CPU tensors against dense math.
* The hot-path names of the reference's utils/common.py (evaluate_dataset, evaluate_ref_conv),
  utils/evaluate_dataset.py and ns/preconditioner/PyAMG.py resolve to this package's functions
  (the table in test_alias_table; the reference's files themselves are not part of this
  repository and are not read). tests/test_gpu_callers.py runs those call sequences on the
  device."""
import sys

import numpy as np
import pytest
import scipy.sparse as sp


@pytest.fixture
def compat(monkeypatch):
    import mlamg.compat
    for name in list(sys.modules):
        if name == "ns" or name.startswith("ns.") or name == "pyamg" or name.startswith("pyamg."):
            monkeypatch.delitem(sys.modules, name)
    installed = mlamg.compat.install(pyamg=True)
    yield installed
    mlamg.compat.uninstall(installed)


def test_alias_table(compat):
    import mlamg.graph
    import mlamg.multigrid
    import mlamg.sparse
    import mlamg.sparse_tensor
    import mlamg.strength
    import ns.lib.graph
    import ns.lib.multigrid
    import ns.lib.sparse
    import ns.lib.sparse_tensor
    import pyamg
    import pyamg.aggregation
    import pyamg.graph
    import pyamg.relaxation.relaxation
    import pyamg.strength
    assert ns.lib.multigrid.amg_2_v is mlamg.multigrid.amg_2_v
    assert ns.lib.graph.modified_bellman_ford is mlamg.graph.modified_bellman_ford
    assert ns.lib.graph.lloyd_aggregation is mlamg.graph.lloyd_aggregation
    assert ns.lib.sparse.scipy_to_torch is mlamg.sparse.to_torch_sparse
    assert ns.lib.sparse_tensor.to_scipy is mlamg.sparse.to_scipy
    assert pyamg.aggregation.lloyd_aggregation is mlamg.graph.pyamg_lloyd_aggregation
    assert pyamg.graph.lloyd_cluster is mlamg.graph.lloyd_cluster
    assert pyamg.graph.bellman_ford is mlamg.graph.bellman_ford
    assert (pyamg.strength.evolution_strength_of_connection
            is mlamg.strength.evolution_strength_of_connection)
    assert callable(pyamg.relaxation.relaxation.gauss_seidel)
    # the rest of the callers' hot path: utils/common.py:40-111, utils/evaluate_dataset.py:59-101
    assert (ns.lib.multigrid.smoothed_aggregation_jacobi
            is mlamg.multigrid.smoothed_aggregation_jacobi)
    assert ns.lib.graph.nearest_center_to_agg is mlamg.graph.nearest_center_to_agg
    assert ns.lib.sparse.torch_to_scipy is mlamg.sparse.to_scipy
    # the PyAMG PC's solver (ns/preconditioner/PyAMG.py:94) and its pieces
    import mlamg.pyamg_compat.aggregation as agg
    assert pyamg.aggregation.smoothed_aggregation_solver is agg.smoothed_aggregation_solver
    assert callable(pyamg.aggregation.standard_aggregation)
    assert callable(pyamg.aggregation.fit_candidates)
    assert callable(pyamg.strength.symmetric_strength_of_connection)
    assert callable(pyamg.relaxation.relaxation.block_gauss_seidel)
    A = sp.identity(4, format="csr")
    for bad in ({"aggregate": "lloyd"}, {"smooth": "energy"}, {"strength": "classical"},
                {"coarse_solver": "splu"}, {"keep": True}):
        with pytest.raises(NotImplementedError):  # before any device call
            pyamg.aggregation.smoothed_aggregation_solver(A, **bad)


def test_sparse_tensor_mirror():
    import torch
    from mlamg import sparse_tensor as st
    rs = np.random.RandomState(0)
    A = (sp.random(9, 7, density=0.3, random_state=rs, format="coo") + sp.eye(9, 7)).tocoo()
    B = sp.random(7, 5, density=0.4, random_state=rs, format="coo")
    At = torch.sparse_coo_tensor(np.vstack([A.row, A.col]), A.data, A.shape).coalesce()
    Bt = torch.sparse_coo_tensor(np.vstack([B.row, B.col]), B.data, B.shape).coalesce()
    assert np.allclose(st.spspmm(At, Bt).to_dense().numpy(), (A @ B).toarray(), rtol=1e-14)
    X = rs.randn(7, 3)
    assert np.allclose(st.spmm(At, torch.as_tensor(X)).numpy(), A @ X, rtol=1e-14)
    assert np.array_equal(st.spT(At).to_dense().numpy(), A.toarray().T)
    d = st.diag(At)
    assert d.dtype == torch.float32 and d.shape == (7,)
    assert np.array_equal(d.numpy(), np.diag(A.toarray())[:7].astype(np.float32)
                          + np.where(np.diag(A.toarray())[:7] == 0, 1, 0))
    S = st.to_scipy(At)
    assert sp.isspmatrix_csr(S) and np.array_equal(S.toarray(), A.toarray())
