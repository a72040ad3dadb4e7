"""GPU, one process, world sizes 2, 3 and 8: the distributed executor of csrc/dhier.hip — halo
packs and exchanges, restriction into owned coarse rows, P-halos aliased to the level below's
buffers, the allgather of coarse segments, the replicated coarse cycle, the norm all-reduce —
run with every rank a host thread on its own stream of the same GPU, over the in-process loopback
transport (mlamg_loop_group; RCCL refuses two ranks on one device). Every rank's owned iterate
must equal the single-GPU iterate bit for bit, and the residual history must agree (only the
norm's summation order differs). The RCCL calls themselves are the loopback's counterparts, one
for one (xsend/xrecv/xgroup_*/xallreduce_sum, comm.hip's transport)."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    A = problems.poisson_3d_7pt(36)
    H = Hierarchy.build(A, alpha=0.1, max_coarse=200)
    assert H.n_levels >= 3
    return A, H


def _run(A, H, world, min_rows, ncyc=6, tol=None, b=None, x0=None, K=None,
         overlap_min_rows=100000, overlap=True):
    import torch
    from mlamg.distributed import DistributedHierarchy, LoopbackGroup
    n = A.shape[0]
    group = LoopbackGroup(world)
    try:
        Ds = [DistributedHierarchy(H, group.comms[r], min_rows=min_rows, A_host=A,
                                   max_partitioned=K, overlap_min_rows=overlap_min_rows)
              for r in range(world)]
        for D in Ds:
            D.set_cycle_graph(False)
            D.set_coarse_graph(False)
            D.set_overlap(overlap)
        bs = [torch.as_tensor(b[D.lo:D.hi]).cuda() for D in Ds]
        xs = [D.new_x(torch.as_tensor(x0[D.lo:D.hi])) for D in Ds]
        torch.cuda.synchronize()
        out = [None] * world
        errs = []

        def work(r):
            try:
                torch.cuda.set_device(0)
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    h = Ds[r].cycle(bs[r], xs[r], ncyc, tol=tol)
                    s.synchronize()
                    out[r] = (xs[r][: Ds[r].n_own].cpu().numpy(), h)
            except Exception as e:  # surfaces in the main thread
                errs.append((r, e))

        th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in th), "a rank did not finish"
        assert not errs, errs
        return Ds, out
    finally:
        torch.cuda.synchronize()
        Ds = None
        group.close()


@pytest.mark.parametrize("world,K", [(2, 1), (2, None), (3, 2), (5, 1), (8, 1), (8, 2), (8, None)])
def test_loopback_distributed_cycle_bitwise(setup, world, K):
    import torch
    A, H = setup
    n = A.shape[0]
    x0 = np.random.RandomState(0).randn(n)
    b = np.random.RandomState(1).randn(n)
    xd = torch.as_tensor(x0).cuda()
    h_ref = H.cycle(torch.as_tensor(b).cuda(), xd, 6, use_graph=False)
    x_ref = xd.cpu().numpy()
    Ds, out = _run(A, H, world, 0, b=b, x0=x0, K=K)
    assert Ds[0].K == (K or len(H.levels))
    for D, (x_own, h) in zip(Ds, out):
        assert np.array_equal(x_own, x_ref[D.lo:D.hi]), f"rank {D.comm.rank} of {world}, K={D.K}"
        np.testing.assert_allclose(h, h_ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("world,K,overlap", [(2, None, True), (3, 2, True), (8, None, True),
                                             (3, None, False)])
def test_loopback_overlap_split_bitwise(setup, world, K, overlap):
    """Every local operator split into boundary | interior | boundary rows (overlap_min_rows=0):
    the exchange runs on the executor's communication stream while the interior rows run, the
    boundary rows after it. The iterate stays bitwise the single-GPU iterate (and with the
    splits present but overlap off)."""
    import torch
    A, H = setup
    n = A.shape[0]
    x0 = np.random.RandomState(7).randn(n)
    b = np.random.RandomState(8).randn(n)
    xd = torch.as_tensor(x0).cuda()
    h_ref = H.cycle(torch.as_tensor(b).cuda(), xd, 6, use_graph=False)
    x_ref = xd.cpu().numpy()
    Ds, out = _run(A, H, world, 0, b=b, x0=x0, K=K, overlap_min_rows=0, overlap=overlap)
    # interior rows exist on every rank's fine operator, so every rank split it
    for D in Ds:
        assert any(s["level"] == 0 and s["op"] == "A" for s in D.splits), D.splits
    if world <= 3:  # thick slabs: the restriction / prolongation are split as well
        assert sum(len(D.splits) for D in Ds) >= 2 * world
    for D, (x_own, h) in zip(Ds, out):
        assert np.array_equal(x_own, x_ref[D.lo:D.hi]), f"rank {D.comm.rank} of {world}, K={D.K}"
        np.testing.assert_allclose(h, h_ref, rtol=1e-12, atol=0)


def test_loopback_tolerance_stop(setup):
    import torch
    A, H = setup
    n = A.shape[0]
    b = np.random.RandomState(2).randn(n)
    x0 = np.zeros(n)
    tol = 1e-6 * float(np.linalg.norm(b))
    xd = torch.zeros(n, dtype=torch.float64, device="cuda")
    h_ref = H.cycle(torch.as_tensor(b).cuda(), xd, 50, tol=tol, use_graph=False)
    Ds, out = _run(A, H, 4, 0, ncyc=50, tol=tol, b=b, x0=x0)
    for D, (x_own, h) in zip(Ds, out):
        assert len(h) == len(h_ref) < 50  # every rank stops after the same cycle
        assert np.array_equal(x_own, xd.cpu().numpy()[D.lo:D.hi])


def test_loopback_refuses_graph_capture(setup):
    import torch
    from mlamg import _lib
    from mlamg.distributed import DistributedHierarchy, LoopbackGroup
    A, H = setup
    group = LoopbackGroup(1)
    try:
        D = DistributedHierarchy(H, group.comms[0], min_rows=0, A_host=A)
        D.set_cycle_graph(True)
        xe = D.new_x(torch.zeros(A.shape[0], dtype=torch.float64))
        with pytest.raises(_lib.MlamgError):
            D.cycle(torch.zeros(A.shape[0], dtype=torch.float64, device="cuda"), xe, 2)
        del D
    finally:
        group.close()


@pytest.mark.slow
def test_loopback_c4_world8_bench_partition():
    """The bench's own configuration at world 8 (C4 216^3, level 0 aggregated in the reference's
    push order and relabelled in seed order, levels with >= 50,000 rows partitioned, per-rank
    autotuned local kernels), eager loopback cycles: every rank's iterate bitwise the
    single-GPU iterate after 3 cycles."""
    import torch
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    A = problems.poisson_3d_7pt(216)
    H = Hierarchy.build(A, alpha=0.1, strength_mode="invabs", max_coarse=2000,
                        aggregation="reference", coarse_order="sorted")
    n = A.shape[0]
    x0 = np.random.RandomState(0).randn(n)
    x0 /= np.linalg.norm(x0)
    b = np.zeros(n)
    xd = torch.as_tensor(x0).cuda()
    h_ref = H.cycle(torch.zeros(n, dtype=torch.float64, device="cuda"), xd, 3, use_graph=True)
    x_ref = xd.cpu().numpy()
    del xd
    Ds, out = _run(A, H, 8, 50000, ncyc=3, b=b, x0=x0)
    assert Ds[0].K == 3
    # the fine operator of every rank is split (two z-planes of boundary rows, one on the ends)
    for D in Ds:
        s0 = [s for s in D.splits if s["level"] == 0 and s["op"] == "A"]
        # the interior part's kernel is an autotune pick among exact-order formats, timed while
        # 8 rank threads share the GPU: which one wins is noise-dependent, the result is not
        assert s0 and s0[0]["formats"][1] is not None, D.splits
    # the row-pair encoder accepts every rank's fine local operator (it is timed; the pick
    # itself is the same noise-dependent contest as above)
    for D in Ds:
        assert any(k.startswith("rowpat") for k in D.tuning[0].get("us", {})), D.tuning[0]
    # every rank's local kernel is a member of its global operator's family (exact order or
    # canonical vector order), so the per-rank timing contest cannot change a bit
    def fam(f):
        return "vector" if f.startswith("vector") else "exact"
    for D in Ds:
        for l in range(D.K):
            glob = {"A": H.levels[l].A, "P": H.levels[l].P, "R": H.levels[l].R}
            for k, t in zip("APR", D.tuning[3 * l:3 * l + 3]):
                assert fam(t["chosen"]) == fam(glob[k].get_format()[0]), (l, k, t["chosen"])
    for D, (x_own, h) in zip(Ds, out):
        assert np.array_equal(x_own, x_ref[D.lo:D.hi]), f"rank {D.comm.rank}"
        np.testing.assert_allclose(h, h_ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("world", (3, 8))
def test_loopback_reference_aggregation(world):
    """The distributed executor on a hierarchy whose level 0 is the reference's push-order
    aggregation relabelled in seed order (bench.py's setting): bitwise the single-GPU iterate;
    with the reference's own column order (seeds unsorted) the partition is refused."""
    import torch
    from mlamg import problems
    from mlamg.distributed import DistributedHierarchy, LoopbackGroup
    from mlamg.hierarchy import Hierarchy
    A = problems.poisson_3d_7pt(30)
    n = A.shape[0]
    H = Hierarchy.build(A, alpha=0.1, max_coarse=200, aggregation="reference",
                        coarse_order="sorted")
    x0 = np.random.RandomState(3).randn(n)
    b = np.random.RandomState(4).randn(n)
    xd = torch.as_tensor(x0).cuda()
    h_ref = H.cycle(torch.as_tensor(b).cuda(), xd, 5, use_graph=False)
    x_ref = xd.cpu().numpy()
    Ds, out = _run(A, H, world, 0, ncyc=5, b=b, x0=x0)
    for D, (x_own, h) in zip(Ds, out):
        assert np.array_equal(x_own, x_ref[D.lo:D.hi]), f"rank {D.comm.rank} of {world}"
        np.testing.assert_allclose(h, h_ref, rtol=1e-12, atol=0)
    Hs = Hierarchy.build(A, alpha=0.1, max_coarse=200, aggregation="reference",
                         coarse_order="seed")
    group = LoopbackGroup(2)
    try:
        with pytest.raises(ValueError):
            DistributedHierarchy(Hs, group.comms[0], min_rows=0, A_host=A)
    finally:
        group.close()


@pytest.mark.parametrize("world", (6, 8))
def test_loopback_ranks_with_empty_coarse_parts(world):
    """A problem so small that coarse levels have fewer rows than ranks: some ranks own no rows
    (or no coarse segment) on a partitioned level; empty halos, packs and operators must still
    line up, and every rank's iterate stays bitwise."""
    import torch
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    A = problems.poisson_3d_7pt(12)
    H = Hierarchy.build(A, alpha=0.1, max_coarse=10)
    n = A.shape[0]
    x0 = np.random.RandomState(5).randn(n)
    b = np.random.RandomState(6).randn(n)
    xd = torch.as_tensor(x0).cuda()
    h_ref = H.cycle(torch.as_tensor(b).cuda(), xd, 4, use_graph=False)
    x_ref = xd.cpu().numpy()
    Ds, out = _run(A, H, world, 0, ncyc=4, b=b, x0=x0)
    sizes = [[p["hi"] - p["lo"] for p in D.parts] for D in Ds]
    segs = [int(D.c_hi[D.comm.rank] - D.c_lo[D.comm.rank]) for D in Ds]
    assert min(min(s) for s in sizes) == 0 or min(segs) == 0, (sizes, segs)
    for D, (x_own, h) in zip(Ds, out):
        assert np.array_equal(x_own, x_ref[D.lo:D.hi]), f"rank {D.comm.rank}: {sizes}, {segs}"
        np.testing.assert_allclose(h, h_ref, rtol=1e-12, atol=0)


def test_sync_formats_makes_replicas_bitwise():
    """What sync_formats does at N > 1: each rank autotunes its own replica of the hierarchy
    (timings, hence CSR-vector widths, may differ), then applies rank 0's format list; the
    replicas must then cycle bit for bit alike (the replicated coarse levels rely on it)."""
    import torch
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    A = problems.poisson_3d_7pt(40)
    H0 = Hierarchy.build(A, alpha=0.1, max_coarse=100)
    H1 = Hierarchy.build(A, alpha=0.1, max_coarse=100, coarse_format="exact")
    # a replica whose timings went another way on every operator (the autotune alone may or may
    # not pick differently on a given box)
    H1.set_formats([{k: (("sell", 1) if v[0] != "sell" else ("csr_stream", 0)) for k, v in lv.items()}
                    for lv in H0.formats()])
    assert all(a[k][0] != b[k][0] for a, b in zip(H0.formats(), H1.formats()) for k in a)
    H1.set_formats(H0.formats())
    assert H1.formats() == H0.formats()
    n = A.shape[0]
    x0 = np.random.RandomState(3).randn(n)
    b = torch.as_tensor(np.random.RandomState(4).randn(n)).cuda()
    xa, xb = torch.as_tensor(x0).cuda(), torch.as_tensor(x0).cuda()
    ha = H0.cycle(b, xa, 4)
    hb = H1.cycle(b, xb, 4)
    assert torch.equal(xa, xb) and np.array_equal(ha, hb)
