"""CPU: the two host-side pieces of FullAggNet.forward_population. PopulationWeights holds a whole
population as one fp32 (P, total) matrix whose slices are what fitness.weights_as_dict hands
load_state_dict, member by member and parameter by parameter, rounding included; a
PopulationBatch of m members has the layout of GraphBatch(As * m), field for field, made from the
base batch's arrays. No GPU: device="cpu"."""
import numpy as np
import pytest


def _As():
    from mlamg import problems
    return [problems.poisson_1d(1), problems.poisson_2d_5pt(5), problems.poisson_2d_5pt(7, 9),
            problems.jump_2d(12, problems.voronoi_jumps(np.random.RandomState(0)))]


def _net():
    import torch
    from mlamg import gnn
    torch.manual_seed(0)
    return gnn.FullAggNet(dim=8, num_conv=2, iterations=2)


def _population(net):
    """float64 rows that are no float32 numbers: the upload has to round them."""
    from mlamg import fitness
    w0 = fitness.weights_as_vector(net).astype(np.float64)
    rs = np.random.RandomState(3)
    pop = np.stack([w0, w0 + rs.uniform(-0.05, 0.05, w0.size), w0 * 1.1 + 1e-9])
    assert not np.array_equal(pop[1], pop[1].astype(np.float32).astype(np.float64))
    return pop


def test_population_weights_are_weights_as_dict():
    import torch
    from mlamg import fitness, gnn
    net = _net()
    pop = _population(net)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    pw = gnn.PopulationWeights(net, pop)
    total = sum(v.numel() for v in before.values())
    assert pw.members == 3 and pw.pstride == total
    assert pw.data.dtype == torch.float32 and tuple(pw.data.shape) == (3, total)
    assert pw.data.is_contiguous()
    params = dict(net.named_parameters())
    assert list(pw.layout) == list(before)
    for m in range(3):
        ref = fitness.weights_as_dict(net, pop[m])
        for name, want in ref.items():
            got = pw.view(name, m)
            assert got.dtype == want.dtype and got.shape == want.shape, (m, name)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (m, name)
            assert got.is_contiguous()
            # a view into the matrix: member m's tensor lies m * pstride floats past member 0's
            assert got.data_ptr() == pw.view(name).data_ptr() + 4 * m * pw.pstride, (m, name)
    for name, p in params.items():  # what a layer asks for: the member-0 view, by parameter
        assert pw(p).data_ptr() == pw.view(name).data_ptr() and pw(p).shape == p.shape, name
    assert pw(None) is None
    with pytest.raises(KeyError):
        pw(torch.zeros(3))
    sub = pw.rows(1, 3)  # the members of a later pass
    assert sub.members == 2 and sub.pstride == total
    for name, p in params.items():
        assert sub(p).data_ptr() == pw.view(name, 1).data_ptr(), name
    for k, v in net.state_dict().items():  # the model itself is not touched
        assert torch.equal(v, before[k]), k
    assert gnn.OWN.pstride == 0 and gnn.OWN(params[name]).data_ptr() == params[name].data_ptr()


def test_population_weights_refusals():
    from mlamg import gnn
    net = _net()
    pop = _population(net)
    with pytest.raises(ValueError, match="entries"):
        gnn.PopulationWeights(net, pop[:, :-1])
    with pytest.raises(ValueError, match="P >= 1"):
        gnn.PopulationWeights(net, pop[:0])
    with pytest.raises(ValueError, match="P >= 1"):
        gnn.PopulationWeights(net, pop[0])  # one flat vector is not a population


def test_population_batch_is_the_repeated_batch():
    import torch
    from mlamg import gnn
    As = _As()
    base = gnn.GraphBatch(As, device="cpu")
    pop = gnn.PopulationBatch(base, 3)
    ref = gnn.GraphBatch(As * 3, device="cpu")
    assert (pop.members, pop.member_n, pop.member_E) == (3, base.n, base.E)
    assert (base.members, base.member_n, base.member_E) == (1, base.n, base.E)
    assert (pop.nb, pop.n, pop.E, pop.fe) == (ref.nb, ref.n, ref.E, ref.fe)
    assert pop.As is base.As  # nothing repeated on the host
    for name in ("seg", "eseg"):
        a, b = getattr(pop, name), getattr(ref, name)
        assert a.host.dtype == np.int64 and np.array_equal(a.host, b.host), name
        assert torch.equal(a.dev, b.dev), name
    for name in ("src", "tgt", "tptr", "teid", "edge_attr", "x", "crow", "edge_index"):
        a, b = getattr(pop, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.is_contiguous(), name
        assert torch.equal(a, b), name
    assert np.array_equal(pop.sizes, ref.sizes)
    assert torch.equal(pop.node_gid, ref.node_gid)
    assert np.array_equal(pop.k_ptr(0.3).host, ref.k_ptr(0.3).host)
    assert pop.k_ptr(0.3) is pop.k_ptr(0.3) and pop.k_ptr(0.3) is not base.k_ptr(0.3)
    # cached on the base batch; a with_x copy of the base gets its own input, repeated
    assert base.population(3) is base.population(3)
    x = np.arange(base.n, dtype=np.float32)
    px = base.with_x(x).population(3)
    assert torch.equal(px.x.reshape(-1), torch.as_tensor(np.tile(x, 3)))
    assert torch.equal(base.population(3).x, ref.x)
    # the cache keeps the two sizes used last (a full pass and a shorter last one)
    three, two = base.population(3), base.population(2)
    assert base.population(3) is three and base.population(2) is two
    base.population(1)  # drops 3, the one used before 2
    assert base.population(2) is two and base.population(3) is not three
    one = gnn.PopulationBatch(base, 1)
    assert torch.equal(one.tptr, base.tptr) and torch.equal(one.teid, base.teid)


def test_population_batch_refusals():
    from mlamg import gnn
    base = gnn.GraphBatch(_As(), device="cpu")
    with pytest.raises(ValueError, match="at least one member"):
        gnn.PopulationBatch(base, 0)
    with pytest.raises(ValueError, match="int32"):
        gnn.PopulationBatch(base, 2 ** 31 // base.E + 1)
    with pytest.raises(ValueError, match="base GraphBatch"):
        gnn.PopulationBatch(gnn.PopulationBatch(base, 2), 2)
