"""GPU: population-stacked FullAggNet inference. The three member-indexed kernels
(mlamg_gnn_linear_pop, mlamg_gnn_nnconv_pop, mlamg_gnn_edge_mlp_pop) against the single-weight
entry points on every member's rows or edges alone with that member's tensors; their refusals;
FullAggNet.forward_population against forward_stack member by member after load_state_dict; the
split into passes; mlamg.fitness.evaluate_population against evaluate_dataset.

No tolerance appears: every comparison is bitwise (int32 views of the floats) against an entry
point that tests/test_gpu_gnn_kernels.py and tests/test_gpu_gnn_batch.py pin to float64
references. Every output is filled with NaN before a call, so an entry a kernel does not write
fails the comparison. Weights are views into a wider (members, total) matrix, so the member
stride is larger than any tensor."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _Weights:
    """Tensors of the given shapes for every member, as views into one (members, total) matrix
    with a few unused floats before, between and behind them."""

    def __init__(self, torch, rs, members, shapes, lo=-0.5, hi=0.5):
        self.at, at = {}, 3
        for name, shape in shapes.items():
            self.at[name] = (at, shape)
            at += int(np.prod(shape)) + 2
        self.pstride = at + 5
        self.data = torch.as_tensor(rs.uniform(lo, hi, (members, self.pstride))
                                    .astype(np.float32)).cuda()

    def view(self, name, member=0):
        at, shape = self.at[name]
        return self.data[member, at:at + int(np.prod(shape))].view(shape)

    def own(self, name, member):
        """Member's tensor in a block of its own, for the single entry."""
        return self.view(name, member).clone()


def _rand(torch, rs, *shape):
    return torch.as_tensor(rs.uniform(-1.0, 1.0, shape).astype(np.float32)).cuda()


# -------------------------------------------------------------------------------------- linear
def _linear_variants(N):
    """(with b, act, beta, rc): every combination the issue names."""
    return [(wb, act, beta, rc) for wb in (False, True) for act in (0, 1) for beta in (0.0, 1.0)
            for rc in (0, 1, N)]


@pytest.mark.parametrize("members", (1, 3))
@pytest.mark.parametrize("M", (1, 5, 33, 257))
@pytest.mark.parametrize("K,N", ((1, 8), (8, 8), (17, 1), (160, 64)))
def test_linear_pop(torch_cuda, K, N, M, members):
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    rs = np.random.RandomState(1000 * K + 10 * N + M + members)
    w = _Weights(torch, rs, members, dict(W=(N, K), b=(N,)))
    assert w.pstride > K * N
    X = _rand(torch, rs, members * M, K)
    Y0 = _rand(torch, rs, members * M, N)
    seen = set()
    for wb, act, beta, rc in _linear_variants(N):
        if (wb, act, beta, rc if rc != N else -1) in seen:  # N == 1: rc = N is rc = 1
            continue
        seen.add((wb, act, beta, rc if rc != N else -1))
        R = _rand(torch, rs, members * M, rc) if rc else None
        Y = Y0.clone() if beta else torch.full_like(Y0, NAN)
        call("mlamg_gnn_linear_pop", ptr(X), M, members, K, ptr(w.view("W")),
             ptr(w.view("b")) if wb else None, w.pstride, N, act, beta, ptr(R), rc, ptr(Y),
             stream_ptr())
        for p in range(members):
            rows = slice(p * M, (p + 1) * M)
            Xp, Wp, bp = X[rows].clone(), w.own("W", p), w.own("b", p)
            Rp = R[rows].clone() if rc else None
            Yp = Y0[rows].clone() if beta else torch.full((M, N), NAN, device="cuda")
            call("mlamg_gnn_linear", ptr(Xp), M, K, ptr(Wp), ptr(bp) if wb else None, N, act,
                 beta, ptr(Rp), rc, ptr(Yp), stream_ptr())
            assert not bool(Yp.isnan().any())
            assert _same(Y[rows], Yp), (K, N, M, members, p, wb, act, beta, rc)
    if members > 1:  # the members' weights differ, and so do their rows (same X in both)
        Xs = X[:M].repeat(members, 1)
        Y = torch.full_like(Y0, NAN)
        call("mlamg_gnn_linear_pop", ptr(Xs), M, members, K, ptr(w.view("W")), None, w.pstride,
             N, 0, 0.0, None, 0, ptr(Y), stream_ptr())
        assert not torch.equal(Y[:M], Y[M:2 * M])


@pytest.mark.parametrize("M", (5, 257))
@pytest.mark.parametrize("K,N", ((8, 8), (17, 1), (160, 64)))
def test_linear_pop_shared_weights(torch_cuda, K, N, M):
    """pstride = 0: every member reads the same tensors, so the call is one mlamg_gnn_linear
    over the whole stack."""
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    rs = np.random.RandomState(K + N + M)
    members = 3
    W, b = _rand(torch, rs, N, K), _rand(torch, rs, N)
    X, R = _rand(torch, rs, members * M, K), _rand(torch, rs, members * M, N)
    Y = torch.full((members * M, N), NAN, device="cuda")
    call("mlamg_gnn_linear_pop", ptr(X), M, members, K, ptr(W), ptr(b), 0, N, 1, 0.0, ptr(R), N,
         ptr(Y), stream_ptr())
    Z = torch.full_like(Y, NAN)
    call("mlamg_gnn_linear", ptr(X), members * M, K, ptr(W), ptr(b), N, 1, 0.0, ptr(R), N,
         ptr(Z), stream_ptr())
    assert not bool(Z.isnan().any()) and _same(Y, Z)


# ------------------------------------------------------------------------ NNConv and edge model
MEMBERS = 3


@pytest.fixture(scope="module")
def stacks(torch_cuda):
    """The base stack of the issue — poisson_2d_5pt(5) (25 rows, 105 edges) and
    poisson_2d_5pt(18) (324 rows) — and its population stack of three members."""
    from mlamg import gnn, problems
    base = gnn.GraphBatch([problems.poisson_2d_5pt(5), problems.poisson_2d_5pt(18)])
    assert base.seg.host.tolist() == [0, 25, 349] and base.eseg.host[1] == 105
    assert base.n % 4 and base.E % 64 and base.E % 4  # no member ends on a tile boundary
    return base, gnn.PopulationBatch(base, MEMBERS)


@pytest.mark.parametrize("Fin,Fout,fe", ((1, 8, 1), (8, 8, 2), (8, 1, 2), (64, 64, 2)))
def test_nnconv_pop(torch_cuda, stacks, Fin, Fout, fe):
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    base, pop = stacks
    n, E = base.n, base.E
    rs = np.random.RandomState(100 * Fin + 10 * Fout + fe)
    w = _Weights(torch, rs, MEMBERS, dict(L1=(4, fe), c1=(4,), L2=(16, 4), c2=(16,),
                                          L3=(Fin * Fout, 16), c3=(Fin * Fout,), bias=(Fout,)))
    X, ea = _rand(torch, rs, MEMBERS * n, Fin), _rand(torch, rs, MEMBERS * E, fe).abs()
    root = _rand(torch, rs, MEMBERS * n, Fout)
    names = ("L1", "c1", "L2", "c2", "L3", "c3")
    for act, rc in ((0, 0), (1, 1), (1, Fout)):
        R = _rand(torch, rs, MEMBERS * n, rc) if rc else None
        msg = torch.full((MEMBERS * E, Fout), NAN, device="cuda")
        Y = torch.full((MEMBERS * n, Fout), NAN, device="cuda")
        call("mlamg_gnn_nnconv_pop", ptr(pop.tptr), ptr(pop.teid), ptr(pop.src), ptr(ea), E,
             MEMBERS, fe, *(ptr(w.view(k)) for k in names), w.pstride, ptr(X), n, Fin, Fout,
             ptr(root), ptr(w.view("bias")), act, ptr(R), rc, ptr(msg), ptr(Y), stream_ptr())
        for p in range(MEMBERS):
            rows, edges = slice(p * n, (p + 1) * n), slice(p * E, (p + 1) * E)
            own = [w.own(k, p) for k in names]
            Xp, eap, rootp, biasp = X[rows].clone(), ea[edges].clone(), root[rows].clone(), \
                w.own("bias", p)
            Rp = R[rows].clone() if rc else None
            msgp = torch.full((E, Fout), NAN, device="cuda")
            Yp = torch.full((n, Fout), NAN, device="cuda")
            call("mlamg_gnn_nnconv", ptr(base.tptr), ptr(base.teid), ptr(base.src), ptr(eap), E,
                 fe, *(ptr(t) for t in own), ptr(Xp), n, Fin, Fout, ptr(rootp), ptr(biasp), act,
                 ptr(Rp), rc, ptr(msgp), ptr(Yp), stream_ptr())
            assert not bool(Yp.isnan().any()) and not bool(msgp.isnan().any())
            assert _same(msg[edges], msgp), (Fin, Fout, fe, p, "msg")
            assert _same(Y[rows], Yp), (Fin, Fout, fe, p, act, rc)
    # the same inputs in every member: the outputs still differ, because the weights do
    Xs, eas, roots = X[:n].repeat(MEMBERS, 1), ea[:E].repeat(MEMBERS, 1), root[:n].repeat(MEMBERS, 1)
    call("mlamg_gnn_nnconv_pop", ptr(pop.tptr), ptr(pop.teid), ptr(pop.src), ptr(eas), E, MEMBERS,
         fe, *(ptr(w.view(k)) for k in names), w.pstride, ptr(Xs), n, Fin, Fout, ptr(roots),
         ptr(w.view("bias")), 0, None, 0, ptr(msg), ptr(Y), stream_ptr())
    assert not torch.equal(Y[:n], Y[n:2 * n]) and not torch.equal(Y[n:2 * n], Y[2 * n:])


@pytest.mark.parametrize("F,fe,H,C", ((8, 2, 8, 2), (1, 2, 8, 1), (64, 2, 64, 2)))
def test_edge_mlp_pop(torch_cuda, stacks, F, fe, H, C):
    torch = torch_cuda
    from mlamg._lib import call, ptr, stream_ptr
    base, pop = stacks
    n, E = base.n, base.E
    rs = np.random.RandomState(100 * F + 10 * H + C)
    w = _Weights(torch, rs, MEMBERS, dict(W1=(H, 2 * F + fe), b1=(H,), g=(H,), beta=(H,),
                                          W2=(C, H), b2=(C,)))
    names = ("W1", "b1", "g", "beta", "W2", "b2")
    X, ea = _rand(torch, rs, MEMBERS * n, F), _rand(torch, rs, MEMBERS * E, fe).abs()

    def pop_call(X, ea, act, R, rc, out):
        v = {k: ptr(w.view(k)) for k in names}
        call("mlamg_gnn_edge_mlp_pop", ptr(pop.src), ptr(pop.tgt), ptr(X), F, ptr(ea), fe, E,
             MEMBERS, v["W1"], v["b1"], H, v["g"], v["beta"], v["W2"], v["b2"], w.pstride, C,
             act, ptr(R), rc, ptr(out), stream_ptr())

    for act, rc in ((0, 0), (1, 1), (1, C)):
        R = _rand(torch, rs, MEMBERS * E, rc) if rc else None
        out = torch.full((MEMBERS * E, C), NAN, device="cuda")
        pop_call(X, ea, act, R, rc, out)
        for p in range(MEMBERS):
            rows, edges = slice(p * n, (p + 1) * n), slice(p * E, (p + 1) * E)
            o = {k: w.own(k, p) for k in names}
            Xp, eap = X[rows].clone(), ea[edges].clone()
            Rp = R[edges].clone() if rc else None
            outp = torch.full((E, C), NAN, device="cuda")
            call("mlamg_gnn_edge_mlp", ptr(base.src), ptr(base.tgt), ptr(Xp), F, ptr(eap), fe, E,
                 ptr(o["W1"]), ptr(o["b1"]), H, ptr(o["g"]), ptr(o["beta"]), ptr(o["W2"]),
                 ptr(o["b2"]), C, act, ptr(Rp), rc, ptr(outp), stream_ptr())
            assert not bool(outp.isnan().any())
            assert _same(out[edges], outp), (F, fe, H, C, p, act, rc)
    out = torch.full((MEMBERS * E, C), NAN, device="cuda")
    pop_call(X[:n].repeat(MEMBERS, 1), ea[:E].repeat(MEMBERS, 1), 0, None, 0, out)
    assert not torch.equal(out[:E], out[E:2 * E]) and not torch.equal(out[E:2 * E], out[2 * E:])


# ------------------------------------------------------------------------------------ refusals
def _einval(torch, name, *args):
    from mlamg import _lib
    conv = [_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(_lib.lib, name)(*conv, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.MLAMG_EINVAL, (name, rc)


def test_linear_pop_refusals(torch_cuda):
    torch = torch_cuda
    M, K, N = 5, 8, 8
    X = torch.ones((3 * M, 161), device="cuda")
    W = torch.ones((3, N * 161), device="cuda")
    Y = torch.full((3 * M, N), NAN, device="cuda")
    f0 = ctypes.c_float(0.0)

    def refused(M=M, members=3, K=K, W=W, pstride=N * 161):
        _einval(torch, "mlamg_gnn_linear_pop", X, M, members, K, W, None, pstride, N, 0, f0,
                None, 0, Y)
        assert bool(Y.isnan().all())

    refused(members=0)
    refused(members=65536)
    refused(members=-1)
    refused(M=(2 ** 31 - 1) // 3 + 1)  # members * M >= 2^31 - 1
    refused(M=2 ** 31 - 1, members=1)
    refused(M=2 ** 62)  # the product would wrap
    refused(K=161)
    refused(K=0)
    refused(W=None)
    refused(pstride=-1)
    # the largest member count and M == 0 are accepted: no launch, nothing written
    from mlamg._lib import call, stream_ptr
    call("mlamg_gnn_linear_pop", None, 0, 65535, K, _p(W), None, 0, N, 0, f0, None, 0, None,
         stream_ptr())
    torch.cuda.synchronize()
    assert bool(Y.isnan().all())


def _p(t):
    from mlamg._lib import ptr
    return ptr(t)


def test_nnconv_and_edge_mlp_pop_refusals(torch_cuda, stacks):
    torch = torch_cuda
    base, pop = stacks
    n, E = base.n, base.E

    def z(*shape):
        return torch.zeros(shape, device="cuda")

    # NNConv(8, 8), fe 2
    w = [z(3, 8), z(3, 4), z(3, 64), z(3, 16), z(3, 1024), z(3, 64)]
    X, ea, root, bias = z(3 * n, 8), z(3 * E, 2), z(3 * n, 8), z(3, 8)
    msg = torch.full((3 * E, 8), NAN, device="cuda")
    Y = torch.full((3 * n, 8), NAN, device="cuda")

    def nnconv(E=E, members=3, w=w, pstride=1024, n=n, Fout=8, bias=bias):
        _einval(torch, "mlamg_gnn_nnconv_pop", pop.tptr, pop.teid, pop.src, ea, E, members, 2,
                *w, pstride, X, n, 8, Fout, root, bias, 0, None, 0, msg, Y)
        assert bool(Y.isnan().all()) and bool(msg.isnan().all())

    nnconv(members=0)
    nnconv(members=65536)
    nnconv(E=(2 ** 31 - 1) // 3 + 1)
    nnconv(n=(2 ** 31 - 1) // 3 + 1)
    nnconv(Fout=65)
    nnconv(pstride=-1)
    nnconv(w=w[:4] + [None, w[5]])  # NULL L3
    nnconv(bias=None)

    # smallEdgeModel(2 * 8 + 2 -> 8 -> 2)
    v = [z(3, 8 * 18), z(3, 8), z(3, 8), z(3, 8), z(3, 16), z(3, 2)]
    out = torch.full((3 * E, 2), NAN, device="cuda")

    def edge(E=E, members=3, F=8, H=8, C=2, v=v, pstride=144):
        _einval(torch, "mlamg_gnn_edge_mlp_pop", pop.src, pop.tgt, X, F, ea, 2, E, members, v[0],
                v[1], H, v[2], v[3], v[4], v[5], pstride, C, 0, None, 0, out)
        assert bool(out.isnan().all())

    edge(members=0)
    edge(members=65536)
    edge(E=(2 ** 31 - 1) // 3 + 1)
    edge(F=80)  # 2 F + fe = 162 > 160
    edge(H=65)
    edge(C=5)
    edge(pstride=-1)
    edge(v=[None] + v[1:])  # NULL W1


# ---------------------------------------------------------------------------- forward_population
ALPHA = 0.1
SEED = 11  # of the perturbation; the test asserts that it separates the members


def _population(torch, net, members=3):
    """The net's own vector (member 0) and seeded perturbations of it in +-0.05."""
    from mlamg import fitness
    w0 = fitness.weights_as_vector(net)
    rs = np.random.RandomState(SEED)
    rows = [w0] + [w0 + rs.uniform(-0.05, 0.05, w0.size).astype(np.float32)
                   for _ in range(members - 1)]
    return np.stack(rows)


def _member_parts(torch, st, n, K, nb, p):
    """Member p's part of a population stack's result with the member's offsets taken off:
    (Agg, P, C) as (indptr, indices, data bits), top_k, node_scores bits, failed."""
    out = []
    for key, coff in (("Agg", K), ("P", K), ("C", n)):
        M = st[key].to_scipy()
        a, b = M.indptr[p * n], M.indptr[(p + 1) * n]
        cols = M.indices[a:b] - p * coff
        assert cols.size == 0 or (cols.min() >= 0 and cols.max() < coff), (key, p)
        out.append((M.indptr[p * n:(p + 1) * n + 1] - a, cols, M.data[a:b].view(np.int64)))
    top = st["top_k"].cpu().numpy()
    out.append(top[(top >= p * n) & (top < (p + 1) * n)] - p * n)
    out.append(st["node_scores"][p * n:(p + 1) * n].cpu().numpy().view(np.int32))
    out.append(np.asarray(st["failed"]).reshape(-1, nb)[p])
    return out


def _assert_member(got, ref, where):
    for name, a, b in zip(("Agg", "P", "C"), got[:3], ref[:3]):
        for part, u, v in zip(("indptr", "indices", "data"), a, b):
            assert np.array_equal(u, v), (where, name, part)
    for name, a, b in zip(("top_k", "node_scores", "failed"), got[3:], ref[3:]):
        assert a.dtype == b.dtype and np.array_equal(a, b), (where, name)


def _reference_members(torch, dim, batch, pop, alpha, aggregation):
    """forward_stack(batch) on a second network after load_state_dict of every member."""
    from mlamg import fitness
    from test_gpu_gnn_batch import _net
    ref_net = _net(torch, dim)
    refs = []
    for p in range(pop.shape[0]):
        ref_net.load_state_dict(fitness.weights_as_dict(ref_net, pop[p]))
        st = ref_net.forward_stack(batch, alpha, aggregation)
        refs.append(_member_parts(torch, st, batch.n, int(st["kptr"].host[-1]), batch.nb, 0))
    return refs


@pytest.mark.parametrize("aggregation", ("pyamg", "parallel"))
@pytest.mark.parametrize("dim", (8, 64))
def test_forward_population_is_forward_stack_per_member(torch_cuda, dim, aggregation):
    torch = torch_cuda
    from mlamg import gnn
    from test_gpu_gnn_batch import _four, _net
    net = _net(torch, dim)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    batch = gnn.GraphBatch(_four())
    pop = _population(torch, net)
    st = net.forward_population(batch, pop, ALPHA, aggregation=aggregation)
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k
    n, nb, K = batch.n, batch.nb, int(batch.k_ptr(ALPHA).host[-1])
    assert st["failed"].shape == (3, nb) and st["failed"].dtype == bool
    assert st["Agg"].shape == (3 * n, 3 * K) and st["P"].shape == (3 * n, 3 * K)
    assert st["C"].shape == (3 * n, 3 * n) and st["node_scores"].shape == (3 * n,)
    assert st["kptr"].host.tolist() == np.concatenate(
        [batch.k_ptr(ALPHA).host[:-1] + p * K for p in range(3)] + [[3 * K]]).tolist()
    assert st["seg"].host.tolist() == gnn.PopulationBatch(batch, 3).seg.host.tolist()
    assert st["top_k"].numel() == 3 * K
    refs = _reference_members(torch, dim, batch, pop, ALPHA, aggregation)
    mine = [_member_parts(torch, st, n, K, nb, p) for p in range(3)]
    for p in range(3):
        _assert_member(mine[p], refs[p], (dim, aggregation, p))
    # a condition on the inputs: the members are told apart, so a kernel that ignored the
    # member index could not have passed
    differ = [not (np.array_equal(refs[0][4], refs[p][4])
                   and np.array_equal(refs[0][1][2], refs[p][1][2])) for p in (1, 2)]
    assert all(differ), differ
    assert not st["failed"].any()


def test_forward_population_split_and_x_hook(torch_cuda):
    """members_per_pass = 2 on three members (a pass of two and a pass of one, joined) and = 1
    give the bits of one pass; the x hook reaches every member."""
    torch = torch_cuda
    from mlamg import gnn
    from test_gpu_gnn_batch import _four, _net
    net = _net(torch, 8)
    batch = gnn.GraphBatch(_four())
    pop = _population(torch, net)
    n, nb, K = batch.n, batch.nb, int(batch.k_ptr(ALPHA).host[-1])
    for x in (None, np.random.RandomState(3).uniform(0.5, 1.5, n).astype(np.float32)):
        one = net.forward_population(batch, pop, ALPHA, x=x)
        for chunk in (2, 1):
            split = net.forward_population(batch, pop, ALPHA, x=x, members_per_pass=chunk)
            assert split["failed"].shape == (3, nb)
            assert split["kptr"].host.tolist() == one["kptr"].host.tolist()
            assert split["seg"].host.tolist() == one["seg"].host.tolist()
            for key in ("Agg", "P", "C"):
                a, b = one[key].to_scipy(), split[key].to_scipy()
                assert a.shape == b.shape and np.array_equal(a.indptr, b.indptr), (chunk, key)
                assert np.array_equal(a.indices, b.indices), (chunk, key)
                assert np.array_equal(a.data.view(np.int64), b.data.view(np.int64)), (chunk, key)
            assert torch.equal(one["top_k"], split["top_k"])
            assert _same(one["node_scores"], split["node_scores"])
            assert np.array_equal(one["failed"], split["failed"])
        if x is not None:  # member 0 is the net itself: forward_stack's x hook, bit for bit
            ref = net.forward_stack(batch, ALPHA, x=x)
            _assert_member(_member_parts(torch, one, n, K, nb, 0),
                           _member_parts(torch, ref, n, K, nb, 0), "x")
    with pytest.raises(ValueError):
        net.forward_stack(gnn.PopulationBatch(batch, 2), ALPHA,
                          weights=gnn.PopulationWeights(net, pop))  # three sets, two members


# ------------------------------------------------------------------------------------- fitness
@pytest.mark.parametrize("case", ("four", "failure"))
def test_evaluate_population_is_evaluate_dataset(torch_cuda, case):
    """On the failure batch (alpha = 0.02: one seed per graph) graph 1 scores 1.0 for every
    member and the others are what they are without it."""
    torch = torch_cuda
    from mlamg import fitness, gnn
    from test_gpu_gnn_batch import _failure_batch, _four, _net
    net = _net(torch, 8)
    As, alpha = (_four(), 0.3) if case == "four" else (_failure_batch(), 0.02)
    batch = gnn.GraphBatch(As)
    pop = _population(torch, net)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    conv = fitness.evaluate_population(net, pop, batch, alpha=alpha)
    fit = fitness.population_fitness_stacked(net, pop, batch, alpha=alpha)
    split = fitness.evaluate_population(net, pop, batch, alpha=alpha, members_per_pass=2)
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert conv.dtype == np.float64 and conv.shape == (3, len(As))
    ref_net = _net(torch, 8)
    ref = np.stack([fitness.evaluate_dataset(ref_net, batch, alpha=alpha, weights=w)
                    for w in pop])
    print(f"[gnn-population] conv {case}: {conv.tolist()}")
    assert np.array_equal(conv, ref), (conv, ref)
    assert np.array_equal(split, ref)
    assert np.array_equal(fit, fitness.population_fitness(ref_net, pop, batch, alpha=alpha))
    if case == "failure":
        assert np.all(conv[:, 1] == 1.0)


def test_evaluate_population_cuts_a_refused_batch_by_member(torch_cuda, monkeypatch):
    """The fused two-level solver plans a batch as a whole: one problem outside its slots (here
    a P whose single column has 324 > 256 entries) sends every problem of its batch to the
    per-problem engine. In the loop a batch is one member's problems, so evaluate_population
    must cut a refused joint batch there: member 0 keeps the fused launch it has in the loop.
    A stand-in model hands over the stacked P, so that the members differ exactly in that."""
    torch = torch_cuda
    import scipy.sparse as sp
    from mlamg import fitness, gnn, multigrid, problems
    from mlamg.sparse import DeviceCSR
    As = [problems.poisson_2d_5pt(5), problems.poisson_2d_5pt(18)]
    batch = gnn.GraphBatch(As)

    def blocks(n, width):  # piecewise-constant P: aggregates of `width` consecutive rows
        k = -(-n // width)
        return sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) // width)), shape=(n, k))

    Ps = [blocks(25, 5), blocks(324, 6), blocks(25, 5), blocks(324, 324)]
    stacked = DeviceCSR.from_scipy(sp.block_diag(Ps).tocsr())
    pop = gnn.PopulationBatch(batch, 2)

    class StandIn:
        def eval(self):
            return self

        def forward_population(self, b, population, alpha, aggregation, members_per_pass=None):
            assert b is batch
            kptr = gnn.SegPtr(np.concatenate([[0], np.cumsum([P.shape[1] for P in Ps])]), "cuda")
            return dict(P=stacked, kptr=kptr, seg=pop.seg, failed=np.zeros((2, 2), dtype=bool))

    def start(A):
        x = np.random.RandomState(0).randn(A.shape[1])
        return np.zeros(A.shape[1]), x / np.linalg.norm(x, 2)

    probs = [(As[i % 2], Ps[i].astype(np.float32)) + start(As[i % 2]) for i in range(4)]
    kw = dict(error_tol=1e-6, pre_smoothing_steps=1, post_smoothing_steps=1)
    # the condition on the inputs: the joint batch is refused, member 0's own is not
    assert multigrid.amg_2_v_batch(probs, fallback=False, **kw) is None
    own0 = multigrid.amg_2_v_batch(probs[:2], fallback=False, **kw)
    assert own0 is not None
    assert multigrid.amg_2_v_batch(probs[2:], fallback=False, **kw) is None
    ref = np.array([[r[1] for r in multigrid.amg_2_v_batch(probs[2 * p:2 * p + 2], **kw)]
                    for p in range(2)])
    assert np.array_equal(ref[0], [r[1] for r in own0])
    sizes, real = [], multigrid.amg_2_v_batch

    def recorded(problems, **k):
        if "engine" not in k:  # the function's own call for its per-problem path has it
            sizes.append(len(problems))
        return real(problems, **k)

    monkeypatch.setattr(multigrid, "amg_2_v_batch", recorded)
    conv = fitness.evaluate_population(StandIn(), None, batch)
    print(f"[gnn-population] refused joint batch: conv {conv.tolist()}")
    assert sizes == [4, 2, 2]
    assert np.array_equal(conv, ref)
