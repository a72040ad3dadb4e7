"""GPU: batched FullAggNet inference. The three segmented kernels (mlamg_gnn_instance_norm_seg,
mlamg_gnn_topk_seg, mlamg_bellman_ford_pyamg_seg) against the single-graph entry points on every
segment alone (bitwise) and against the float64 / oracle references; the single entry points as
the segmented ones on one segment (mlamg_gnn_topk on its cached scratch); their refusals; then
FullAggNet.forward_batch against forward() graph by graph, bitwise in every tensor, and
mlamg.fitness against the loop forward() -> amg_2_v().

No tolerance is used where the batched and the single path are compared: both run the same
arithmetic in the same order. The only tolerance is the rule of tests/test_gpu_gnn_kernels.py for
InstanceNorm against float64, err <= max(4 err_ref32, 4 * 2^-24 * scale), per segment."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 255, 256, 257, 1000)  # one row, a partial stride, one stride, several strides


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _seg(torch, sizes):
    from mlamg import gnn
    return gnn.SegPtr(np.concatenate([[0], np.cumsum(sizes)]), "cuda")


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------- segmented norm
def _norm_input(F):
    """Per segment the channels of oracle.gnn_kernel_cases.instance_norm_cases: std_f (u_f + z),
    z standardised over the segment's rows, |u_f| <= 9.5 (the mean up to 9.5 sigma off zero);
    the one-row segment is constant by itself, and for F >= 3 the last channel of the 256-row
    segment is the exact constant 1/256."""
    rs = np.random.RandomState(1000 + F)
    Xs, consts = [], []
    for n in SIZES:
        z = rs.randn(n, F)
        z = (z - z.mean(axis=0)) / z.std(axis=0) if n >= 2 else np.zeros((n, F))
        X = (rs.uniform(0.5, 2.0, F) * (rs.uniform(-9.5, 9.5, F) + z)).astype(np.float32)
        const = np.full(F, n == 1)
        if n == 256 and F >= 3:
            X[:, F - 1] = np.float32(1.0 / n)
            const[F - 1] = True
        Xs.append(X)
        consts.append(const)
    return Xs, consts


@pytest.mark.parametrize("F", (1, 8, 64))
def test_instance_norm_seg(torch_cuda, F):
    torch = torch_cuda
    from mlamg import gnn
    from oracle import gnn_kernel_cases as gc
    Xs, consts = _norm_input(F)
    seg = _seg(torch, SIZES)
    X = torch.as_tensor(np.concatenate(Xs)).cuda()
    Y = gnn.instance_norm_seg(X, seg)
    assert Y.shape == X.shape and bool(torch.isfinite(Y).all())
    for g, n in enumerate(SIZES):
        a = int(seg.host[g])
        mine = Y[a:a + n]
        single = gnn.instance_norm(X[a:a + n].clone())
        assert torch.equal(mine.view(torch.int32), single.view(torch.int32)), (F, n)
        c = dict(kernel="instance_norm", id=f"seg-n{n}-F{F}", n=n, F=F, X=Xs[g], eps=1e-5,
                 const=consts[g])
        for label, err, err32, scale, tol, ok in gc.judge(c, {"Y": mine.cpu().numpy()}):
            print(f"[gnn-batch] inorm_seg n{n} F{F} {label}: err {err:.3e} err_ref32 {err32:.3e} "
                  f"scale {scale:.3e} tol {tol:.3e}")
            assert ok, (F, n, label, err, tol)
        if consts[g].any():  # a constant channel: mean == the constant exactly, so x - mean == 0
            assert bool((mine[:, torch.as_tensor(consts[g]).cuda()] == 0).all()), (F, n)


# ------------------------------------------------------------------------------ segmented top-k
def _topk_scores():
    """Planted ties: [-0.0, +0.0] alone in a segment, one segment all equal, ~70 % exact zeros of
    both signs elsewhere."""
    rs = np.random.RandomState(77)
    out = []
    for n in SIZES:
        if n == 2:
            s = np.array([-0.0, 0.0])
        elif n == 256:
            s = np.full(n, 0.75)
        else:
            s = np.where(rs.uniform(size=n) < 0.7, rs.choice([0.0, -0.0], n),
                         rs.uniform(-1.0, 1.0, n))
        out.append(s.astype(np.float32))
    return out


def _k_choices(n):
    return (0, 1, int(np.ceil(0.1 * n)), n)


@pytest.mark.parametrize("shift", (0, 1, 2, 3))
def test_topk_seg(torch_cuda, shift):
    """k_g in {0, 1, ceil(0.1 n_g), n_g}, a different choice in neighbouring segments."""
    torch = torch_cuda
    from mlamg import gnn
    from oracle import gnn_kernels_ref as kref
    scores = _topk_scores()
    ks = [_k_choices(n)[(g + shift) % 4] for g, n in enumerate(SIZES)]
    seg, kptr = _seg(torch, SIZES), _seg(torch, ks)
    s = torch.as_tensor(np.concatenate(scores)).cuda()
    vec, idx = gnn.topk_vec_seg(s, seg, kptr)
    torch.cuda.synchronize()
    assert vec.dtype == torch.float32 and idx.dtype == torch.int32
    assert idx.numel() == sum(ks)
    for g, (n, k) in enumerate(zip(SIZES, ks)):
        a, q = int(seg.host[g]), int(kptr.host[g])
        svec, sidx = gnn.topk_vec(s[a:a + n].clone(), k)
        rvec, ridx = kref.topk(scores[g], k)
        mine_v, mine_i = vec[a:a + n], idx[q:q + k]
        assert torch.equal(mine_v.view(torch.int32), svec.view(torch.int32)), (g, k)
        assert torch.equal(mine_i, sidx + a), (g, k)
        assert np.array_equal(mine_v.cpu().numpy().view(np.uint32), rvec.view(np.uint32)), (g, k)
        assert np.array_equal(mine_i.cpu().numpy() - a, ridx), (g, k)
        assert int((mine_v == 1).sum()) == k and int((mine_v == 0).sum()) == n - k


# ------------------------------------------------------------- one segment is the single call
@pytest.mark.parametrize("n", SIZES)
def test_one_segment_is_the_single_call(torch_cuda, n):
    """The single entry points run the segmented kernels with null offsets: offsets [0, n] given
    explicitly are the same call, bit for bit."""
    torch = torch_cuda
    from mlamg import gnn
    g = SIZES.index(n)
    seg = _seg(torch, [n])
    for F in (1, 8, 64):
        X = torch.as_tensor(_norm_input(F)[0][g]).cuda()
        stacked, single = gnn.instance_norm_seg(X, seg), gnn.instance_norm(X)
        assert torch.equal(stacked.view(torch.int32), single.view(torch.int32)), (n, F)
    s = torch.as_tensor(_topk_scores()[g]).cuda()
    for k in _k_choices(n):
        vec, idx = gnn.topk_vec_seg(s, seg, _seg(torch, [k]))
        svec, sidx = gnn.topk_vec(s, k)
        assert torch.equal(vec.view(torch.int32), svec.view(torch.int32)), (n, k)
        assert idx.dtype == sidx.dtype and torch.equal(idx, sidx), (n, k)


def test_topk_single_on_cached_scratch(torch_cuda):
    """mlamg_gnn_topk keeps its sort storage in a cached block: a larger earlier call leaves
    nothing behind in a smaller later one, and the same input gives the same bits again. The
    entry synchronises: the results are read on another (non-blocking) stream straight after it
    returns, with no synchronisation in between."""
    torch = torch_cuda
    from mlamg._lib import call, ptr
    from oracle import gnn_kernels_ref as kref
    scores = dict(zip(SIZES, _topk_scores()))
    work, side = torch.cuda.Stream(), torch.cuda.Stream()

    def run(s_np, k, with_idx=True):
        s = torch.as_tensor(s_np).cuda()
        vec = torch.full((s.numel(),), float("nan"), dtype=torch.float32, device="cuda")
        idx = torch.full((max(k, 1),), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # the inputs are in place before `work` reads them
        call("mlamg_gnn_topk", ptr(s), int(s.numel()), int(k), ptr(vec),
             ptr(idx) if with_idx else None, ctypes.c_void_p(work.cuda_stream))
        with torch.cuda.stream(side):
            v, i = vec.cpu().numpy(), idx.cpu().numpy()[:k]
        rvec, ridx = kref.topk(s_np, k)
        assert np.array_equal(v.view(np.uint32), rvec.view(np.uint32)), (s_np.size, k)
        if with_idx:
            assert np.array_equal(i, ridx), (s_np.size, k)
        else:
            assert np.all(idx.cpu().numpy() == -1)  # NULL idx: nothing is written for it
        return v

    first = run(scores[1000], 100)
    run(np.array([-0.0, 0.0], dtype=np.float32), 1)
    run(scores[257], 257)
    last = run(scores[1000], 100, with_idx=False)
    assert np.array_equal(first.view(np.uint32), last.view(np.uint32))


def test_topk_single_refusals(torch_cuda):
    torch = torch_cuda
    s = torch.arange(5, dtype=torch.float32, device="cuda")
    vec = torch.full((5,), float("nan"), dtype=torch.float32, device="cuda")
    idx = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    _einval(torch, "mlamg_gnn_topk", s, 5, 6, vec, idx)  # k > n
    _einval(torch, "mlamg_gnn_topk", s, 2 ** 31 - 1, 0, vec, idx)  # past the int32 node ids
    assert bool(vec.isnan().all()) and idx.cpu().tolist() == [-1] * 6


# ---------------------------------------------------------------------- segmented Bellman-Ford
def _bf_graphs():
    """(name, float32-weight CSR with sorted rows, sorted seeds)."""
    from mlamg import problems
    rs = np.random.RandomState(11)
    A = problems.poisson_2d_5pt(23).tocoo()
    out = []

    def add(name, w, rows, cols, shape, seeds):
        G = sp.coo_matrix((np.asarray(w, dtype=np.float32), (rows, cols)), shape=shape).tocsr()
        G.sort_indices()
        assert G.nnz == len(rows) and G.has_canonical_format
        out.append((name, G, np.sort(np.asarray(seeds, dtype=np.int32))))

    add("random", rs.uniform(0.1, 2.0, A.nnz), A.row, A.col, A.shape,
        rs.permutation(A.shape[0])[:40])
    add("equal", np.ones(A.nnz), A.row, A.col, A.shape, rs.permutation(A.shape[0])[:40])
    up = A.col >= A.row
    add("nonsym", rs.uniform(0.05, 1.0, up.sum()), A.row[up], A.col[up], A.shape, [17, 400])
    B = problems.poisson_3d_7pt(11).tocoo()  # 1331 rows: more than one trip of the 1024 threads
    add("int3d", rs.randint(0, 3, B.nnz) + 0.0, B.row, B.col, B.shape,
        rs.permutation(B.shape[0])[:30])
    T = sp.block_diag([problems.poisson_2d_5pt(6), problems.poisson_1d(5)]).tocoo()
    add("two_comp", np.ones(T.nnz), T.row, T.col, T.shape, [3])
    add("equal_again", np.ones(A.nnz), A.row, A.col, A.shape, [0, 528])
    return out


def _stack(Gs):
    """The block-diagonal stack by concatenation (explicit zeros kept), fp64 values."""
    sizes = [G.shape[0] for G in Gs]
    seg = np.concatenate([[0], np.cumsum(sizes)])
    eoff = np.concatenate([[0], np.cumsum([G.nnz for G in Gs])])
    indptr = np.concatenate([[0]] + [G.indptr[1:] + eoff[g] for g, G in enumerate(Gs)])
    indices = np.concatenate([G.indices + seg[g] for g, G in enumerate(Gs)])
    data = np.concatenate([G.data.astype(np.float64) for G in Gs])
    n = int(seg[-1])
    return sp.csr_matrix((data, indices.astype(np.int32), indptr.astype(np.int32)),
                         shape=(n, n)), seg


@pytest.mark.parametrize("lds", ("0", "1"))
@pytest.mark.parametrize("fp64", (False, True))
def test_bellman_ford_pyamg_seg(torch_cuda, oracle, monkeypatch, fp64, lds):
    """lds: distances and labels kept in global memory / in LDS while a graph sweeps (the library
    picks LDS by itself when the largest graph fits); the bits are the same."""
    torch = torch_cuda
    monkeypatch.setenv("MLAMG_BF_SEG_LDS", lds)
    from mlamg import graph
    from mlamg.sparse import DeviceCSR
    cases = _bf_graphs()
    Gs = [G for _, G, _ in cases]
    S, seg = _stack(Gs)
    Sd = DeviceCSR.from_scipy(S, check=False)
    assert Sd.nnz == sum(G.nnz for G in Gs)
    plan = graph.BellmanFordSegPlan(Sd, seg)
    seed_ptr = np.concatenate([[0], np.cumsum([len(s) for _, _, s in cases])])
    seeds = torch.as_tensor(np.concatenate([s + seg[g] for g, (_, _, s) in enumerate(cases)])
                            .astype(np.int32)).cuda()
    dt = np.float64 if fp64 else np.float32
    d, z, sweeps = graph.bellman_ford_pyamg_seg_device(plan, Sd, seeds, seed_ptr, fp64=fp64)
    d2, z2, sweeps2 = graph.bellman_ford_pyamg_seg_device(plan, Sd, seeds, seed_ptr, fp64=fp64)
    assert torch.equal(d, d2) and torch.equal(z, z2) and np.array_equal(sweeps, sweeps2)
    d, z = d.cpu().numpy(), z.cpu().numpy()
    assert d.dtype == dt
    for g, (name, G, s) in enumerate(cases):
        a, n = int(seg[g]), G.shape[0]
        Gd = DeviceCSR.from_scipy(sp.csr_matrix((G.data.astype(np.float64), G.indices, G.indptr),
                                                shape=G.shape), check=False)
        ds, zs, sw = graph.bellman_ford_pyamg_device(Gd, torch.as_tensor(s).cuda(), fp64=fp64)
        ds, zs = ds.cpu().numpy(), zs.cpu().numpy()
        dr, zr, swr = oracle.pyamg_bellman_ford(G, s, dtype=dt)
        local = np.where(z[a:a + n] >= 0, z[a:a + n] - a, -1)
        assert np.array_equal(d[a:a + n], ds) and np.array_equal(d[a:a + n], dr), name
        assert np.array_equal(local, zs) and np.array_equal(local, zr), name
        assert int(sweeps[g]) == sw == swr, (name, sweeps[g], sw, swr)
        if name == "two_comp":  # the 1-D component has no seed
            assert np.all(local[36:] == -1) and np.all(d[a + 36:a + n] == np.finfo(dt).max)
            assert np.all(local[:36] == 3)


# ------------------------------------------------------------------------------------ refusals
def _einval(torch, name, *args):
    from mlamg import _lib
    conv = [_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(_lib.lib, name)(*conv, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.MLAMG_EINVAL, (name, rc)


@pytest.mark.parametrize("mirror", (True, False))
def test_refusals_leave_outputs_untouched(torch_cuda, mirror):
    """mirror: the offsets' host copy is passed / the entry reads the device copy back itself."""
    torch = torch_cuda
    from mlamg import problems
    from mlamg._lib import call, ptr, stream_ptr
    from mlamg.sparse import DeviceCSR
    nan = float("nan")

    def host(p):
        return _hp(p.host) if mirror else None

    # an empty segment in the norm
    seg = _seg(torch, [3, 0, 2])
    X = torch.ones((5, 4), dtype=torch.float32, device="cuda")
    Y = torch.full((5, 4), nan, dtype=torch.float32, device="cuda")
    _einval(torch, "mlamg_gnn_instance_norm_seg", X, seg.dev, host(seg), 3, 4,
            ctypes.c_float(1e-5), Y)
    assert bool(Y.isnan().all())
    # k_g > n_g (the total would fit)
    seg, kptr = _seg(torch, [3, 4]), _seg(torch, [4, 1])
    s = torch.arange(7, dtype=torch.float32, device="cuda")
    vec = torch.full((7,), nan, dtype=torch.float32, device="cuda")
    idx = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    _einval(torch, "mlamg_gnn_topk_seg", s, seg.dev, host(seg), kptr.dev, host(kptr), 2, vec, idx)
    assert bool(vec.isnan().all()) and idx.cpu().tolist() == [-1] * 5
    # a coupling across two segments: no plan
    A = problems.poisson_1d(6)
    Ad = DeviceCSR.from_scipy(A)
    seg = _seg(torch, [3, 3])
    h = ctypes.c_void_p()
    _einval(torch, "mlamg_bellman_ford_pyamg_seg_plan_create", Ad.handle, seg.dev, host(seg), 2,
            ctypes.byref(h))
    assert not h.value
    # a seed outside its segment (inside the stack)
    B = abs(sp.block_diag([problems.poisson_1d(3), problems.poisson_1d(3)]).tocsr())
    Bd = DeviceCSR.from_scipy(B)
    call("mlamg_bellman_ford_pyamg_seg_plan_create", Bd.handle, ptr(seg.dev), host(seg), 2,
         ctypes.byref(h), stream_ptr())
    try:
        sptr = _seg(torch, [1, 1])
        seeds = torch.as_tensor(np.array([1, 2], dtype=np.int32)).cuda()  # 2 is graph 0's row
        dist = torch.full((6,), nan, dtype=torch.float32, device="cuda")
        near = torch.full((6,), -7, dtype=torch.int32, device="cuda")
        sweeps = np.full(2, -9, dtype=np.int32)
        _einval(torch, "mlamg_bellman_ford_pyamg_seg", h, Bd.handle, seeds, sptr.dev, host(sptr),
                0, dist, near, _hp(sweeps))
        assert bool(dist.isnan().all()) and near.cpu().tolist() == [-7] * 6
        # the same plan still serves a valid call
        seeds = torch.as_tensor(np.array([1, 5], dtype=np.int32)).cuda()
        call("mlamg_bellman_ford_pyamg_seg", h, Bd.handle, ptr(seeds), ptr(sptr.dev), host(sptr),
             0, ptr(dist), ptr(near), _hp(sweeps), stream_ptr())
        assert near.cpu().tolist() == [1, 1, 1, 5, 5, 5]
        # negative weights in graph 1 only: no fixed point within n_g + 2 = 5 sweeps there; the
        # message names the graph, graph 0 is complete
        N = sp.block_diag([abs(problems.poisson_1d(3)), problems.poisson_1d(3)]).tocsr()
        Nd = DeviceCSR.from_scipy(N)
        from mlamg import _lib
        rc = _lib.lib.mlamg_bellman_ford_pyamg_seg(h, Nd.handle, ptr(seeds), ptr(sptr.dev),
                                                   host(sptr), 0, ptr(dist), ptr(near),
                                                   _hp(sweeps), stream_ptr())
        assert rc == _lib.MLAMG_EINVAL and b"graph 1" in _lib.lib.mlamg_last_error()
        assert near.cpu().tolist()[:3] == [1, 1, 1] and sweeps.tolist() == [2, 5]
    finally:
        call("mlamg_bellman_ford_pyamg_seg_plan_destroy", h)


# ------------------------------------------------------------------- forward_batch vs forward
def _net(torch, dim):
    """The live network of test_fullaggnet_forward_end_to_end: seeded, positive biases."""
    from mlamg import gnn
    torch.manual_seed(0)
    net = gnn.FullAggNet(dim=dim, num_conv=2, iterations=2)
    for mod in net.modules():
        if isinstance(mod, torch.nn.Linear) and mod.bias is not None:
            mod.bias.data.uniform_(0.05, 0.3)
    return net.cuda()


def _four():
    from mlamg import problems
    return [problems.poisson_2d_5pt(5), problems.poisson_2d_5pt(18),  # 18^2 = 324 > 256 rows
            problems.jump_2d(12, problems.voronoi_jumps(np.random.RandomState(0))),
            problems.poisson_2d_5pt(7, 9)]


def _same_entry(torch, got, ref, where):
    assert isinstance(got, tuple) and len(got) == len(ref) == 5, where
    for name, a, b in zip(("agg", "P", "bf_weights", "cluster_centers", "node_weights"), got, ref):
        w = (where, name)
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), w
        assert a.is_sparse == b.is_sparse, w
        if a.is_sparse:
            assert a.is_coalesced() and b.is_coalesced(), w
            assert a.indices().dtype == b.indices().dtype, w
            assert torch.equal(a.indices(), b.indices()), w
            av, bv = a.values(), b.values()
            assert av.dtype == bv.dtype == torch.float32, w
            assert torch.equal(av.view(torch.int32), bv.view(torch.int32)), w
        elif a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), w
        else:
            assert torch.equal(a, b), w


@pytest.mark.parametrize("aggregation", ("pyamg", "pyamg64", "parallel"))
@pytest.mark.parametrize("dim", (8, 64))
def test_forward_batch_is_forward_per_graph(torch_cuda, dim, aggregation):
    torch = torch_cuda
    from mlamg import gnn
    net = _net(torch, dim)
    As = _four()
    batch = gnn.GraphBatch(As)
    out = net.forward_batch(batch, 0.1, aggregation=aggregation)
    assert len(out) == len(As)
    for g, A in enumerate(As):
        ref = net.forward(A, 0.1, aggregation=aggregation)
        assert ref[0].shape == (A.shape[0], int(np.ceil(0.1 * A.shape[0])))
        _same_entry(torch, out[g], ref, (dim, aggregation, g))
    again = net.forward_batch(batch, 0.1, aggregation=aggregation)  # cached plan and weights
    for g in range(len(As)):
        _same_entry(torch, again[g], out[g], (dim, aggregation, g, "again"))


def test_forward_batch_x_hook(torch_cuda):
    torch = torch_cuda
    from mlamg import gnn
    net = _net(torch, 8)
    As = _four()
    batch = gnn.GraphBatch(As)
    rs = np.random.RandomState(3)
    xs = [rs.uniform(0.5, 1.5, A.shape[0]).astype(np.float32) for A in As]
    out = net.forward_batch(batch, 0.1, x=np.concatenate(xs))
    for g, A in enumerate(As):
        _same_entry(torch, out[g], net.forward(A, 0.1, x=xs[g]), ("x", g))
    assert torch.equal(batch.x[:25], gnn.Graph(As[0]).x)  # the batch keeps its own input


def _failure_batch():
    from mlamg import problems
    return [problems.poisson_2d_5pt(6),
            sp.block_diag([problems.poisson_2d_5pt(6), problems.poisson_1d(3)]).tocsr(),
            problems.poisson_2d_5pt(5)]


def test_forward_batch_failure_entry(torch_cuda):
    """alpha = 0.02: one seed per graph, so the seedless component of graph 1 is unreached."""
    torch = torch_cuda
    from mlamg import gnn
    net = _net(torch, 8)
    As = _failure_batch()
    batch = gnn.GraphBatch(As)
    out = net.forward_batch(batch, 0.02)
    assert out[1] is None
    for g in (0, 2):
        _same_entry(torch, out[g], net.forward(As[g], 0.02), ("failure", g))
    with pytest.raises(KeyError):
        net.forward(As[1], 0.02)
    with pytest.raises(KeyError, match="graph 1"):
        net.forward_batch(batch, 0.02, strict=True)
    par = net.forward_batch(batch, 0.02, aggregation="parallel")  # no failure entry there
    assert all(e is not None for e in par)
    _same_entry(torch, par[1], net.forward(As[1], 0.02, aggregation="parallel"), ("parallel", 1))


# ------------------------------------------------------------------------------------- fitness
def _loop_conv(net, As, alpha):
    from mlamg import multigrid, sparse
    conv = np.ones(len(As))
    for g, A in enumerate(As):
        try:
            P = sparse.to_scipy(net.forward(A, alpha)[1])
        except KeyError:
            continue
        n = A.shape[1]
        x = np.random.RandomState(0).randn(n)
        x /= np.linalg.norm(x, 2)
        conv[g] = multigrid.amg_2_v(A, P, np.zeros(n), x, error_tol=1e-6)[1]
    conv[np.isnan(conv)] = 1.0
    return conv


def test_evaluate_dataset_is_the_loop(torch_cuda):
    torch = torch_cuda
    from mlamg import fitness, gnn
    net = _net(torch, 8)
    for As, alpha in ((_four(), 0.3), (_four(), 0.1), (_failure_batch(), 0.02)):
        batch = gnn.GraphBatch(As)
        conv = fitness.evaluate_dataset(net, batch, alpha=alpha)
        ref = _loop_conv(net, As, alpha)
        print(f"[gnn-batch] conv alpha {alpha}: {conv.tolist()}")
        assert conv.dtype == np.float64 and conv.shape == (len(As),)
        assert np.array_equal(conv, ref), (alpha, conv, ref)
    assert conv[1] == 1.0  # the failed graph of the failure batch


def test_population_fitness_and_weight_vector(torch_cuda):
    torch = torch_cuda
    from mlamg import fitness, gnn
    net = _net(torch, 8)
    batch = gnn.GraphBatch(_four())
    w0 = fitness.weights_as_vector(net)
    assert w0.dtype == np.float32 and w0.ndim == 1
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    rs = np.random.RandomState(5)
    pop = np.stack([w0, w0 + rs.uniform(0.0, 0.02, w0.size).astype(np.float32),
                    w0 * np.float32(1.1)])
    fit = fitness.population_fitness(net, pop, batch)
    assert fit.shape == (3,)
    # the last row stays loaded: same shapes, the same bits back
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == shapes
    assert np.array_equal(fitness.weights_as_vector(net).view(np.uint32), pop[2].view(np.uint32))
    for i in range(3):
        conv = fitness.evaluate_dataset(net, batch, weights=pop[i])
        assert fit[i] == 1.0 / np.average(conv), i
        assert np.array_equal(fitness.weights_as_vector(net).view(np.uint32),
                              pop[i].view(np.uint32)), i
