"""GPU, one rank: the RCCL distributed executor (csrc/dhier.hip) with 1..all levels partitioned
reproduces the single-GPU V-cycle bit for bit (the multi-rank maps are covered by the gloo
emulation in test_distributed_gloo.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    from mlamg.distributed import Comm
    A = problems.poisson_3d_7pt(24)
    H = Hierarchy.build(A, alpha=0.1, max_coarse=60)
    assert H.n_levels >= 3
    return A, H, Comm(1, 0)


@pytest.mark.parametrize("min_rows", [10**9, 1000, 0])
def test_distributed_single_rank_bitwise(setup, min_rows):
    from mlamg.distributed import DistributedHierarchy
    A, H, comm = setup
    n = A.shape[0]
    D = DistributedHierarchy(H, comm, min_rows=min_rows, A_host=A)
    if min_rows == 0:
        assert D.K == len(H.levels)
    if min_rows == 10**9:
        assert D.K == 1
    x0 = np.random.RandomState(0).randn(n)
    b = torch.as_tensor(np.random.RandomState(1).randn(n)).cuda()
    x = torch.as_tensor(x0).cuda()
    h_ref = H.cycle(b, x, 6, use_graph=False)
    for coarse_graph, cycle_graph in ((False, False), (True, False), (True, True), (False, True)):
        D.set_coarse_graph(coarse_graph)
        D.set_cycle_graph(cycle_graph)
        for rep in range(2):  # the second call replays the captured cycle
            xe = D.new_x(torch.as_tensor(x0))
            h = D.cycle(b, xe, 6)
            assert torch.equal(xe[:n], x), f"K={D.K} graphs={coarse_graph},{cycle_graph}"
            np.testing.assert_allclose(h, h_ref, rtol=1e-12, atol=0)


def test_distributed_tolerance_stop(setup):
    from mlamg.distributed import DistributedHierarchy
    A, H, comm = setup
    n = A.shape[0]
    D = DistributedHierarchy(H, comm, min_rows=0, A_host=A)
    b = torch.as_tensor(np.random.RandomState(2).randn(n)).cuda()
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    h_ref = H.cycle(b, x, 50, tol=1e-6 * float(torch.linalg.norm(b)), use_graph=False)
    for cycle_graph in (False, True):
        D.set_cycle_graph(cycle_graph)
        xe = D.new_x(torch.zeros(n, dtype=torch.float64))
        h = D.cycle(b, xe, 50, tol=1e-6 * float(torch.linalg.norm(b)))
        assert len(h) == len(h_ref) < 50
        assert torch.equal(xe[:n], x)


def test_cached_graphs_survive_changes_to_the_replicated_hierarchy(setup):
    """One executor with both of its graphs cached (the whole-cycle graph of the mlamg_dhier, the
    zero-guess graph of its replicated tail) keeps computing the eager bits while the replicated
    hierarchy it shares operators with is used and changed in between: a captured cycle of H
    itself, set_smoothing to the same values (drops a hierarchy's graphs), and a set_format of a
    tail operator (format epoch: every cached graph is stale). The same three on the executor's
    own tail handle, whose top-level graph is re-keyed while its zero-guess graph is in use."""
    from mlamg import problems
    from mlamg._lib import call, ptr, stream_ptr
    from mlamg.distributed import DistributedHierarchy
    from mlamg.hierarchy import Hierarchy
    _, _, comm = setup
    A = problems.poisson_3d_7pt(20)
    n = A.shape[0]
    H = Hierarchy.build(A, alpha=0.1, max_coarse=100, coarse_format="exact")
    D = DistributedHierarchy(H, comm, min_rows=10**9, A_host=A)
    assert D.K == 1 and len(H.levels) == 2  # the tail is one level and the coarse solve
    rs = np.random.RandomState(5)
    x0 = torch.as_tensor(rs.randn(n))
    b = torch.as_tensor(rs.randn(n)).cuda()
    xe = D.new_x(x0)
    hist = torch.zeros(5, dtype=torch.float64, device="cuda")

    def cycle():  # same b, x and history buffers every time: the executor's graph key holds
        xe[:n].copy_(x0)
        hist.zero_()
        call("mlamg_dhier_vcycle", D.handle, ptr(b), ptr(xe), 5, -1.0, ptr(hist), None,
             stream_ptr())
        return xe[:n].clone(), hist.cpu().numpy()

    D.set_coarse_graph(False)
    D.set_cycle_graph(False)
    x_ref, h_ref = cycle()  # the eager executor, itself bitwise the single-GPU iterate
    x_single = x0.cuda()
    H.cycle(b, x_single, 5, use_graph=False)
    assert torch.equal(x_ref, x_single)

    def check(what):
        x, h = cycle()
        assert torch.equal(x, x_ref) and np.array_equal(h, h_ref), what

    n1 = H.levels[1].A.shape[0]
    b1 = torch.as_tensor(rs.randn(n1)).cuda()

    def tail_cycle(handle, nb):  # a captured top-level cycle on a hierarchy handle
        x = torch.zeros(nb, dtype=torch.float64, device="cuda")
        rhs = b if nb == n else b1
        call("mlamg_hier_vcycle", handle, ptr(rhs), ptr(x), 2, -1.0, None, None, 1, stream_ptr())

    for coarse_graph, cycle_graph in ((True, True), (True, False)):
        D.set_coarse_graph(coarse_graph)
        D.set_cycle_graph(cycle_graph)
        check("first")
        check("replay")
        tail_cycle(H.handle, n)
        check("after a captured cycle of H")
        call("mlamg_hier_set_smoothing", H.handle, 1, 1)
        check("after H.set_smoothing")
        tail_cycle(D.coarse, n1)
        check("after a captured top-level cycle of the tail")
        call("mlamg_hier_set_smoothing", D.coarse, 1, 1)
        check("after set_smoothing on the tail")
        H.levels[1].A.set_format("csr_stream" if cycle_graph else "sell")
        check("after set_format")


def test_finalize_replicated_matches_full_build():
    """bench.py's N > 1 setup: every rank builds with finalize=False, rank 0 autotunes and
    broadcasts the formats, every rank then builds its coarse solver (finalize_replicated) —
    the cycle is bitwise that of a hierarchy built in one call (world 1 here; the broadcast is
    the same object list sync_formats used)."""
    from mlamg import problems
    from mlamg.distributed import finalize_replicated
    from mlamg.hierarchy import Hierarchy
    A = problems.poisson_3d_7pt(24)
    n = A.shape[0]
    H1 = Hierarchy.build(A, alpha=0.1, max_coarse=60, aggregation="reference",
                         coarse_order="sorted")
    H2 = Hierarchy.build(A, alpha=0.1, max_coarse=60, aggregation="reference",
                         coarse_order="sorted", finalize=False)
    assert H2.handle is None
    finalize_replicated(H2, 1, 0)
    x0 = np.random.RandomState(0).randn(n)
    b = torch.as_tensor(np.random.RandomState(1).randn(n)).cuda()
    x1, x2 = torch.as_tensor(x0).cuda(), torch.as_tensor(x0).cuda()
    h1 = H1.cycle(b, x1, 5)
    h2 = H2.cycle(b, x2, 5)
    assert np.array_equal(h1, h2) and torch.equal(x1, x2)
