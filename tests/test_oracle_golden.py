"""CPU: pin the oracle (oracle/) against golden vectors produced by the reference itself
(tests/golden/make_golden.py). Bitwise wherever the reference is deterministic scipy/driver code."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden_csr

MATS = ("c1", "p2d", "lap3d", "rnd")


@pytest.mark.parametrize("k", MATS)
def test_csr_matvec_bitwise(golden, oracle, k):
    A = golden_csr(golden, k)
    y = oracle.csr_matvec(A, golden[f"{k}_x"])
    assert np.array_equal(y, golden[f"{k}_Ax"])
    r = golden[f"{k}_b"] - y
    assert np.array_equal(r, golden[f"{k}_resid"])


@pytest.mark.parametrize("k", MATS)
@pytest.mark.parametrize("nu", (1, 2, 5))
def test_jacobi_mg_bitwise(golden, oracle, k, nu):
    A = golden_csr(golden, k)
    x = oracle.jacobi_mg(A, golden[f"{k}_b"], golden[f"{k}_x"].copy(), omega=0.666, nu=nu)
    assert np.array_equal(x, golden[f"{k}_jacobi_nu{nu}"])


def test_sa_prolongator_and_galerkin(golden, oracle):
    A = golden_csr(golden, "c1")
    n = A.shape[0]
    Agg = sp.csr_matrix((np.ones(n), golden["c1_Agg_indices"], golden["c1_Agg_indptr"]))
    # ARPACK starts from a random vector, so omega varies in the last bits between runs
    _, om = oracle.smoothed_aggregation_jacobi(A, Agg)
    assert abs(om - golden["c1_omega"]) <= 1e-12 * golden["c1_omega"]
    P, om = oracle.smoothed_aggregation_jacobi(A, Agg, omega=float(golden["c1_omega"]))
    assert np.array_equal(P.indptr, golden["c1_P_indptr"])
    assert np.array_equal(P.indices, golden["c1_P_indices"])
    assert np.array_equal(P.data, golden["c1_P_data"])
    AH = oracle.galerkin(A, P)
    assert np.array_equal(AH.indptr, golden["c1_AH_indptr"])
    assert np.array_equal(AH.indices, golden["c1_AH_indices"])
    assert np.array_equal(AH.data, golden["c1_AH_data"])


def _P1(golden):
    A = golden_csr(golden, "c1")
    P = sp.csr_matrix((golden["c1_P_data"], golden["c1_P_indices"], golden["c1_P_indptr"]),
                      shape=(A.shape[0], int(golden["c1_Agg_indices"].max()) + 1))
    return A, P


def test_amg_2_v_driver(golden, oracle):
    A, P = _P1(golden)
    n = A.shape[0]
    x0 = np.random.RandomState(0).normal(0, 1, n)
    b0 = np.zeros(n)
    x, conv, err, it = oracle.amg_2_v(A, P, b0, x0, error_tol=1e-10)
    assert np.array_equal(err, golden["c1_amg2v_err_hist"])
    assert conv == golden["c1_amg2v_err_conv"]
    assert np.array_equal(x, golden["c1_amg2v_err_x"])
    x, conv, err, it = oracle.amg_2_v(A, P, b0, x0 / np.linalg.norm(x0), res_tol=1e-10)
    assert np.array_equal(err, golden["c1_amg2v_res_hist"])
    assert conv == golden["c1_amg2v_res_conv"]


def test_conv_factor_quirks(golden, oracle):
    A, P = _P1(golden)
    n = A.shape[0]
    x0 = np.random.RandomState(0).normal(0, 1, n)
    got = [float(oracle.amg_2_v(A, P, np.zeros(n), x0, error_tol=1e-300, max_iter=L)[1])
           for L in range(1, 8)]
    assert np.array_equal(np.array(got), golden["conv_quirk_values"])
    # lengths 1, 3, 4, 5 -> 0 (err_n == 1 divides by zero; len 1 special-cased)
    assert got[0] == 0 and got[2] == 0 and got[3] == 0 and got[4] == 0


def test_mlamg_residual_history(golden, oracle):
    A, P = _P1(golden)
    n = A.shape[0]
    x0 = np.random.RandomState(0).normal(0, 1, n)
    x, hist = oracle.mlamg_amg_2_v(A, P, oracle.mlamg_dinv(A), np.zeros(n), x0, max_iter=8,
                                   amg_rtol=0.0)
    assert np.array_equal(hist, golden["c1_mlamg_hist"])
    assert np.array_equal(x, golden["c1_mlamg_x8"])


@pytest.mark.parametrize("k", ("p2d", "rnd", "lap3d"))
def test_bellman_ford_reference(golden, oracle, k):
    A = golden_csr(golden, k)
    C = sp.csr_matrix((1.0 / np.abs(A.data), A.indices, A.indptr), A.shape)
    seeds = golden[f"{k}_bf_seeds"]
    d, nc, _ = oracle.modified_bellman_ford(C, seeds)
    assert np.array_equal(d, golden[f"{k}_bf_dist"])
    assert np.array_equal(nc, golden[f"{k}_bf_nearest"])
    # order-independent fixed point: canonical distances are the reference's, bit for bit
    dc, lab = oracle.canon_bellman_ford(C, seeds)
    assert np.array_equal(dc, golden[f"{k}_bf_dist"])
    agree = np.mean(lab == golden[f"{k}_bf_nearest"])
    if k == "rnd":  # tie-free random weights: unique shortest paths
        assert agree == 1.0
    else:
        assert agree > 0.5


@pytest.mark.parametrize("k", ("p2d", "rnd", "lap3d"))
def test_nearest_center_to_agg_layout(golden, oracle, k):
    seeds = golden[f"{k}_bf_seeds"]
    Agg = oracle.nearest_center_to_agg(seeds, golden[f"{k}_bf_nearest"]).tocoo()
    idx = golden[f"{k}_agg_idx"]
    assert np.array_equal(Agg.row, idx[0]) and np.array_equal(Agg.col, idx[1])


def test_lloyd_aggregation_driver(golden, oracle):
    A = golden_csr(golden, "rnd")
    C = sp.csr_matrix((1.0 / np.abs(A.data), A.indices, A.indptr), A.shape)
    AggOp, roots, seeds = oracle.lloyd_aggregation(C, ratio=0.1, distance='same', rand=0)
    assert np.array_equal(seeds, golden["rnd_lloyd_seeds"])
    assert np.array_equal(roots, golden["rnd_lloyd_roots"])
    assert np.array_equal(AggOp.indptr, golden["rnd_lloyd_agg_indptr"])
    assert np.array_equal(AggOp.indices, golden["rnd_lloyd_agg_indices"])
    # on tie-free weights the order-independent variant agrees exactly
    AggC, rootsC, _ = oracle.lloyd_aggregation(C, ratio=0.1, distance='same', rand=0, canon=True)
    assert np.array_equal(rootsC, roots)
    assert np.array_equal(AggC.indices, AggOp.indices)


def test_gridio_matches_golden(golden):
    import os
    from mlamg import gridio
    # the reference's demos/laplace_3d.grid, stored unchanged beside the golden vectors
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "laplace_3d.grid")
    A, x, extra = gridio.load_grid(path)
    assert np.array_equal(A.data, golden["lap3d_data"])
    assert np.array_equal(A.indices, golden["lap3d_indices"])
    assert A.shape == (1331, 1331) and A.nnz == 17191


@pytest.mark.parametrize("key", ("n1d", "n2d"))
def test_amg_2_v_singular_driver(golden_singular, oracle, key):
    """multigrid.py:111-210 with singular=True (lsqr coarse solve + mean removal) on Neumann
    problems: the oracle reproduces the reference's history, conv factor and iterate bitwise."""
    g = golden_singular
    A, P = golden_csr(g, f"{key}_A"), golden_csr(g, f"{key}_P")
    kw = {"res_tol": 1e-8} if key == "n1d" else {"error_tol": 1e-9}
    x, conv, err, it = oracle.amg_2_v(A, P, g[f"{key}_b"], g[f"{key}_x0"], singular=True,
                                      max_iter=60, **kw)
    assert np.array_equal(err, g[f"{key}_err"])
    assert conv == g[f"{key}_conv"]
    assert np.array_equal(x, g[f"{key}_x"])


def _pyamg_bf_literal(G, seeds, dt=np.float32):
    """pyamg 4.x graph.bellman_ford + amg_core.bellman_ford, transcribed line by line (numpy
    float32 scalars: every sum rounds to float32 like the <int, float> instantiation)."""
    import scipy.sparse as sp
    G = sp.csr_matrix(G)
    G.sum_duplicates()
    n = G.shape[0]
    x = np.full(n, np.finfo(dt).max, dtype=dt)
    x[seeds] = 0
    z = np.full(n, -1, dtype=np.int32)
    z[seeds] = seeds
    w = G.data.astype(dt)
    sweeps = 0
    while True:
        old = x.copy()
        for i in range(n):
            xi, zi = x[i], z[i]
            for jj in range(G.indptr[i], G.indptr[i + 1]):
                j = G.indices[jj]
                d = dt(w[jj] + x[j])
                if d < xi:
                    xi, zi = d, z[j]
            x[i], z[i] = xi, zi
        sweeps += 1
        if (old == x).all():
            return x, z, sweeps


@pytest.mark.parametrize("kind", ("random", "unit_ties", "disconnected"))
def test_oracle_pyamg_bellman_ford(oracle, kind):
    """oracle.pyamg_bellman_ford (the restatement of the aggregation step FullAggNet runs,
    ns/model/agg_interp.py:475) against a second, independent Python restatement of pyamg 4.x
    (a self-consistency check of two restatements — parity unpinned, pyamg absent): distances, nearest
    seeds (first strictly better in sweep order — ties included) and the sweep count; its
    distances are the order-independent fixed point the device's own Bellman-Ford computes."""
    import scipy.sparse as sp
    from mlamg import problems
    rs = np.random.RandomState(7)
    A = problems.poisson_2d_5pt(11).tocoo()
    if kind == "random":
        w = rs.uniform(0.1, 2.0, A.nnz).astype(np.float32)
    elif kind == "unit_ties":
        w = np.ones(A.nnz, dtype=np.float32)
    else:
        w = rs.uniform(0.1, 2.0, A.nnz).astype(np.float32)
        cut = (A.row < 60) != (A.col < 60)  # two components
        w = w[~cut]
        A = sp.coo_matrix((np.ones(len(w)), (A.row[~cut], A.col[~cut])), shape=A.shape)
    G = sp.coo_matrix((w, (A.row, A.col)), shape=A.shape)
    seeds = np.sort(rs.permutation(A.shape[0])[:12]).astype(np.int32)
    if kind == "disconnected":
        seeds = seeds[seeds < 60]
    d, z, sw = oracle.pyamg_bellman_ford(G, seeds)
    dl, zl, swl = _pyamg_bf_literal(G, seeds)
    assert np.array_equal(d, dl) and np.array_equal(z, zl) and sw == swl
    d64, z64, sw64 = oracle.pyamg_bellman_ford(G, seeds, dtype=np.float64)
    dl, zl, swl = _pyamg_bf_literal(G, seeds, np.float64)
    assert d64.dtype == np.float64
    assert np.array_equal(d64, dl) and np.array_equal(z64, zl) and sw64 == swl
    # canon_bellman_ford pushes along C[i, j] (i -> j); pyamg pulls d_i = min_j G[i, j] + d_j
    dc, _ = oracle.canon_bellman_ford(sp.csr_matrix(G).T.tocsr().astype(np.float64), seeds)
    reach = z >= 0
    assert np.array_equal(d[reach], dc[reach])
    if kind == "disconnected":
        assert not reach.all() and np.all(d[~reach] == np.finfo(np.float32).max)


@pytest.mark.parametrize("k", ("p2d", "lap3d"))
@pytest.mark.parametrize("case", ("unit0", "unit3", "olson"))
def test_lloyd_tie_rich_driver(golden, oracle, k, case):
    """The oracle's pyamg-order lloyd_cluster inside its restated driver against the reference
    driver run around that same restated lloyd_cluster on tie-rich graphs
    (tests/golden/reference_callers.npz): pins the restated DRIVER (seeding, distances, AggOp)
    to the reference's; the cluster kernel is self-consistent only (pyamg absent: unpinned)."""
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_callers.npz")))
    A = golden_csr(golden, k)
    if case == "olson":
        np.random.seed(0)
        C = oracle.strength_measure(A, "olson")
        AggOp, roots, seeds = oracle.lloyd_aggregation(C, ratio=0.1, distance='same', rand=0)
    else:
        C = sp.csr_matrix((np.ones_like(A.data), A.indices, A.indptr), A.shape)
        AggOp, roots, seeds = oracle.lloyd_aggregation(C, ratio=0.1, distance='unit',
                                                       rand=int(case[-1]))
    assert np.array_equal(seeds, g[f"{k}_{case}_seeds"])
    assert np.array_equal(roots, g[f"{k}_{case}_roots"])
    assert np.array_equal(AggOp.indptr, g[f"{k}_{case}_agg_indptr"])
    assert np.array_equal(AggOp.indices, g[f"{k}_{case}_agg_indices"])


def test_reference_aggregates_match_dumb_driver(oracle):
    """oracle.reference_aggregates (the recipe of Hierarchy.build(aggregation='reference'),
    the bench's level-0 aggregation) against the reference's own utils/evaluate_dataset.py
    'dumb' method (:80-90) run here on the caller dataset (tests/golden/reference_callers.npz,
    ed_dumb*): unsorted RandomState(0) seeds, modified_bellman_ford, nearest_center_to_agg —
    the aggregate operator bitwise (indptr, indices). The strength is the loop's olson measure
    (pyamg's evolution restated, global RNG re-seeded as the loop does: parity of that measure
    is unpinned; the aggregation recipe around it is what this pins)."""
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_callers.npz")))
    i = 0
    while f"ds{i}_indptr" in g:
        A = sp.csr_matrix((g[f"ds{i}_data"], g[f"ds{i}_indices"], g[f"ds{i}_indptr"]))
        np.random.seed(0)  # utils/evaluate_dataset.py:70
        C = oracle.strength_measure(A, "olson")
        _, _, Agg = oracle.reference_aggregates(C, A.shape[0], 0.1, 0)
        assert np.array_equal(Agg.indptr, g[f"ed_dumb{i}_agg_indptr"]), i
        assert np.array_equal(Agg.indices, g[f"ed_dumb{i}_agg_indices"]), i
        i += 1
    assert i >= 4
