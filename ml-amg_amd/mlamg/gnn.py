"""GNN inference for learned aggregates and interpolation on the device.

Mirrors ns/model/agg_interp.py: `FullAggNet.forward(A, alpha)` (:432-486) -> AggNet node scores
(TAGConv / InstanceNorm / MLP layers, top-k seeds), CNet (MPNN: NNConv + edge models) edge
weights for Bellman-Ford, the aggregates, PNet (MPNN) edge values P_hat and P = P_hat Agg. The
modules hold their parameters like the reference's (same attribute names and shapes, so a
reference state_dict — e.g. from ns.ga.torch.model_weights_as_dict — loads with
load_state_dict); the forward passes run on csrc/gnn.hip kernels (fp32, like the reference),
not on torch ops. torch_geometric is absent: its layers (TAGConv K=3 with gcn_norm, NNConv aggr
'add' with root weight, InstanceNorm) are restated from its 2.x semantics; the reference's
trained weights are not shipped, so parity is against oracle/gnn_ref.py (a torch restatement
of the same layers) at seeded weights — parity unpinned with respect to torch_geometric itself.

There is one forward pass, `FullAggNet.forward_stack`, on a `GraphBatch`: many graphs stacked
block-diagonally, the per-graph steps (InstanceNorm, top-k, pyamg's sweep) done segment by
segment. A `Graph` is a batch of one, `forward` runs it on that, `forward_batch` on many graphs at
once, every graph's tensors bitwise its own `forward`.
`forward_population` runs the same pass for a whole population of weight vectors at once, on a
`PopulationBatch` (the stack repeated once per individual) with the weights taken from a
`PopulationWeights` matrix instead of the modules: the layers' `run` methods take either source,
and a `GraphBatch` is a population of one member.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr, stream_ptr


def _p(t):
    return ptr(t) if t is not None else None


# ------------------------------------------------------------------------------------ graphs
@functools.lru_cache(maxsize=1024)
def _offsets_on_device(raw, device):
    """int64 offsets (their bytes) as a read-only device tensor. forward() builds a Graph per
    call, so the same few small arrays recur: each is uploaded once."""
    return torch.as_tensor(np.frombuffer(raw, dtype=np.int64).copy()).to(device)


class SegPtr:
    """Segment offsets of a stack, int64[nb + 1] from 0: on the host and on the device (the C
    entry points validate the host copy, the kernels read the device copy, made on first use)."""

    def __init__(self, host, device):
        self.host = np.ascontiguousarray(host, dtype=np.int64)
        self.device = torch.device(device)
        self.nb = int(self.host.size - 1)
        # made once: the layers pass it on every call, and numpy builds .ctypes anew each time
        self.host_ptr = self.host.ctypes.data_as(ctypes.c_void_p)

    @functools.cached_property
    def dev(self):
        return _offsets_on_device(self.host.tobytes(), self.device)


class GraphBatch:
    """Many graphs as one block-diagonal stack, built once per dataset. Per graph the fields are
    graph_from_matrix_basic(A_g) (ns/model/data.py:22-31): edges = A_g's stored entries in
    row-major order (networkx DiGraph order), edge_attr = |a_ij| (fp32), x = 1/n_g. On the stack
    the node ids of graph g are offset by seg.host[g] and the edges follow in graph order — the
    layout of scipy.sparse.block_diag(As) — with the node and edge segment pointers (seg, eseg),
    every node's graph id (node_gid), the cached gcn_norm weights and the cached Bellman-Ford
    level plan (created on first use, on the device).

    Every GNN kernel but InstanceNorm and top-k produces a row or an edge from its own inputs in
    an order that does not depend on where the item sits; those two and pyamg's sequential sweep
    work segment by segment. So every graph's part of a result carries the bits it has when the
    graph runs alone. Every matrix must have canonical format (sorted, duplicate-free rows):
    pyamg would sweep a re-sorted, duplicate-summed copy, which only a Graph on its own does."""

    def __init__(self, As, device=None):
        mats = [sp.csr_matrix(A) for A in As]
        for i, A in enumerate(mats):
            if not A.has_canonical_format:
                raise ValueError(f"matrix {i} of the batch has no canonical format (unsorted or "
                                 "duplicate entries); run it through forward() on its own")
        self._build(mats, device)

    def _build(self, mats, device):
        """Every field, from a list of CSR matrices in any stored order."""
        for i, A in enumerate(mats):
            if A.shape[0] != A.shape[1] or A.shape[0] < 1:
                raise ValueError(f"matrix {i} of the batch is not square and non-empty: {A.shape}")
        if not mats:
            raise ValueError("empty batch")
        dev = torch.device(device or torch.device("cuda", torch.cuda.current_device()))
        sizes = np.array([A.shape[0] for A in mats], dtype=np.int64)
        nnzs = np.array([A.nnz for A in mats], dtype=np.int64)
        seg = np.concatenate([[0], np.cumsum(sizes)])
        eseg = np.concatenate([[0], np.cumsum(nnzs)])
        n, E = int(seg[-1]), int(eseg[-1])
        if n >= 2 ** 31 - 1 or E >= 2 ** 31 - 1:
            raise ValueError("batch exceeds the int32 index range")
        indptr = np.concatenate([[0]] + [A.indptr[1:].astype(np.int64) + eseg[g]
                                         for g, A in enumerate(mats)]).astype(np.int32)
        tgt = np.concatenate([A.indices.astype(np.int64) + seg[g]
                              for g, A in enumerate(mats)]).astype(np.int32)
        src = np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr))
        ea = np.concatenate([np.abs(A.data.astype(np.float32)) for A in mats])[:, None]
        order = np.argsort(tgt, kind="stable")          # each target's edges, ascending source
        tptr = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(np.bincount(tgt, minlength=n), out=tptr[1:])
        self.As = mats
        self.nb, self.n, self.E, self.fe = len(mats), n, E, 1
        self.members, self.member_n, self.member_E = 1, n, E  # one member: the stack itself
        self.sizes = sizes
        self.device = dev
        self.seg, self.eseg = SegPtr(seg, dev), SegPtr(eseg, dev)
        self.crow = torch.as_tensor(indptr, device=dev)
        self.src = torch.as_tensor(src, device=dev)
        self.tgt = torch.as_tensor(tgt, device=dev)
        self.tptr = torch.as_tensor(tptr, device=dev)
        self.teid = torch.as_tensor(order.astype(np.int32), device=dev)
        self.edge_attr = torch.as_tensor(np.ascontiguousarray(ea), device=dev)
        self.x = torch.as_tensor(np.repeat((1.0 / sizes).astype(np.float32), sizes)[:, None],
                                 device=dev)
        self.edge_index = torch.stack([self.src.long(), self.tgt.long()])
        self._shared = {"kptr": {}}  # gcn weights, plan, seed offsets: shared by the copies

    @property
    def node_gid(self):
        """Every node's graph id (int64, on the device), made on first use."""
        if "gid" not in self._shared:
            gid = np.repeat(np.arange(self.nb, dtype=np.int64), self.sizes)
            self._shared["gid"] = torch.as_tensor(gid, device=self.device)
        return self._shared["gid"]

    def _copy(self):
        g = object.__new__(type(self))
        g.__dict__.update(self.__dict__)
        return g

    def with_clusters(self, col):
        """graph_from_matrix(A, Agg) (ns/model/data.py:33-46) from this stack and the device
        aggregate column of every node (-1: none; agg_op.argmax(axis=1) of an empty row is 0):
        edge feature 2 = cluster_adj = 0 if both ends are in the same aggregate, else 1. Shares
        the structure."""
        g = self._copy()
        c = torch.where(col < 0, torch.zeros_like(col), col)
        adj = (c[self.src.long()] != c[self.tgt.long()]).to(torch.float32)
        g.edge_attr = torch.stack([self.edge_attr[:, 0], adj], dim=1).contiguous()
        g.fe = 2
        return g

    def with_x(self, x):
        """The stack with the node input x (n values, graph after graph) instead of 1/n_g."""
        g = self._copy()
        x = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x,
                            dtype=torch.float32)
        g.x = x.reshape(self.n, 1).to(self.device)
        return g

    def csr(self, values):
        """A DeviceCSR on the stacked pattern with the given per-edge values (fp64 copy)."""
        from .sparse import DeviceCSR
        return DeviceCSR.from_torch(self.crow, self.tgt, values.reshape(-1).double().contiguous(),
                                    (self.n, self.n))

    def gcn_weights(self):
        """gcn_norm(edge_index, edge_attr[:, 0]) without self loops (TAGConv normalize=True).
        Edge feature 0 never changes, so the copies share the cached weights."""
        if "gcn" not in self._shared:
            w = self.edge_attr[:, 0].contiguous()
            dis = torch.empty(self.n, dtype=torch.float32, device=w.device)
            wn = torch.empty(self.E, dtype=torch.float32, device=w.device)
            call("mlamg_gnn_gcn_norm", ptr(self.tptr), ptr(self.teid), ptr(self.src),
                 ptr(self.tgt), ptr(w), int(self.n), int(self.E), ptr(dis), ptr(wn), stream_ptr())
            self._shared["gcn"] = wn
        return self._shared["gcn"]

    def _seed_ptr(self, key, ks):
        cache = self._shared["kptr"]
        if key not in cache:
            cache[key] = SegPtr(np.concatenate([[0], np.cumsum(ks())]), self.device)
        return cache[key]

    def k_ptr(self, alpha):
        """Offsets of k_g = ceil(alpha n_g) seeds per graph (SegPtr), cached per alpha."""
        return self._seed_ptr(float(alpha),
                              lambda: [int(np.ceil(alpha * int(m))) for m in self.sizes])

    def seed_ptr(self, k):
        """k as seed offsets: a SegPtr as it is; a stack of one graph also takes its seed count."""
        if isinstance(k, SegPtr):
            return k
        if self.nb != 1:
            raise TypeError("a stack of several graphs takes its seed offsets as a SegPtr")
        return self._seed_ptr(("k", int(k)), lambda: [int(k)])

    def plan(self):
        """The Bellman-Ford level plan of the stacked pattern (graph.BellmanFordSegPlan)."""
        if "plan" not in self._shared:
            from .graph import BellmanFordSegPlan
            pattern = self.csr(torch.zeros(self.E, dtype=torch.float32, device=self.device))
            self._shared["plan"] = BellmanFordSegPlan(pattern, self.seg.host)
        return self._shared["plan"]

    def pyamg_sweep(self, C, seeds, kptr, fp64):
        """pyamg.graph.bellman_ford(C, seeds) per graph, on the cached level plan: (the matrix
        swept — C itself —, every node's nearest seed as a node id of the stack, -1: none)."""
        from .graph import bellman_ford_pyamg_seg_device
        return C, bellman_ford_pyamg_seg_device(self.plan(), C, seeds, kptr.host, fp64=fp64,
                                                seed_ptr_dev=kptr.dev)[1]

    def population(self, members):
        """The `members`-fold PopulationBatch of this stack, cached (its Bellman-Ford plan and
        seed offsets with it: a genetic algorithm asks for the same one every generation), with
        this copy's node input. A replica holds `members` times the batch's device arrays, its
        gcn weights and its plan for as long as it is cached, so the cache keeps the two sizes
        used last — the full pass and the shorter last pass of a split population — and drops
        the older ones. For a with_x copy of the batch the cached replica is used with that
        input repeated, which is redone on every call."""
        cache = self._shared.setdefault("population", {})
        pop = cache.pop(members, None) or PopulationBatch(self, members)
        cache[members] = pop  # most recently used last
        while len(cache) > 2:
            del cache[next(iter(cache))]
        if pop._base_x is not self.x:  # a with_x copy of the batch the cached one was made from
            pop = pop.with_x(self.x.reshape(-1).repeat(members))
        return pop


class PopulationBatch(GraphBatch):
    """`members` equal copies of a GraphBatch end to end, one per individual of a population: the
    layout of GraphBatch(batch.As * members) — member p owns rows [p n, (p + 1) n) and edges
    [p E, (p + 1) E) of the base stack's n rows and E edges (member_n, member_E), ids are ids of
    the whole stack, nb counts every (member, graph) segment, member-major — made from the base
    batch's arrays where that lives, without stacking the matrices again. As is the base batch's
    list (not repeated: every member's graph g is As[g % len(As)]). The seed offsets, the gcn
    weights and the Bellman-Ford plan are its own, cached like a GraphBatch's. The base must be
    a stack of canonical matrices with its original edge feature (a GraphBatch, not a
    with_clusters copy)."""

    def __init__(self, batch, members):
        members = int(members)
        if members < 1:
            raise ValueError(f"a population has at least one member, got {members}")
        if batch.fe != 1 or batch.members != 1:
            raise ValueError("a population stack is made from a base GraphBatch")
        for i, A in enumerate(batch.As):
            if not A.has_canonical_format:
                raise ValueError(f"matrix {i} of the batch has no canonical format (unsorted or "
                                 "duplicate entries)")
        bn, bE, dev = batch.n, batch.E, batch.device
        n, E = members * bn, members * bE
        if members > 65535 or n >= 2 ** 31 - 1 or E >= 2 ** 31 - 1:
            raise ValueError("population stack exceeds 65535 members or the int32 index range")

        def tiled(host, step):  # offsets without the closing entry, member after member
            rep = host[:-1][None, :] + step * np.arange(members, dtype=np.int64)[:, None]
            return np.concatenate([rep.ravel(), [members * step]])

        def shifted(t, step, closed=False):  # a device id / offset array of the base, likewise
            base = t[:-1] if closed else t
            off = torch.arange(members, dtype=torch.int64, device=dev) * step
            out = (base.long()[None, :] + off[:, None]).reshape(-1)
            if closed:
                out = torch.cat([out, out.new_tensor([members * step])])
            return out.to(torch.int32)

        self.As = batch.As
        self.nb, self.n, self.E, self.fe = members * batch.nb, n, E, 1
        self.members, self.member_n, self.member_E = members, bn, bE
        self.sizes = np.tile(batch.sizes, members)
        self.device = dev
        self.seg = SegPtr(tiled(batch.seg.host, bn), dev)
        self.eseg = SegPtr(tiled(batch.eseg.host, bE), dev)
        self.crow = shifted(batch.crow, bE, closed=True)
        self.src = shifted(batch.src, bn)
        self.tgt = shifted(batch.tgt, bn)
        self.tptr = shifted(batch.tptr, bE, closed=True)
        self.teid = shifted(batch.teid, bE)
        self.edge_attr = batch.edge_attr.repeat(members, 1)
        self.x = batch.x.repeat(members, 1)
        self._base_x = batch.x
        self.edge_index = torch.stack([self.src.long(), self.tgt.long()])
        self._shared = {"kptr": {}}


class Graph(GraphBatch):
    """One graph: graph_from_matrix_basic(A) / graph_from_matrix(A, agg) (ns/model/data.py:22-46)
    on the device, a GraphBatch of A alone. A may have any stored order: the edges keep it."""

    def __init__(self, A, agg=None, device=None):
        self._build([sp.csr_matrix(A)], device)
        if agg is not None:
            col = np.asarray(sp.csr_matrix(agg).argmax(axis=1)).ravel()
            clustered = self.with_clusters(torch.as_tensor(col, device=self.device))
            self.edge_attr, self.fe = clustered.edge_attr, clustered.fe

    def pyamg_sweep(self, C, seeds, kptr, fp64):
        """The same with mlamg_bellman_ford_pyamg, which takes a graph of any size. pyamg's
        asgraph turns the COO C (agg_interp.py:471) into csr_matrix: columns sorted, duplicate
        edges summed in C's float32; its sweep visits each row in that order."""
        from .graph import bellman_ford_pyamg_device
        from .sparse import DeviceCSR
        if not self.As[0].has_canonical_format:
            m, Cs = self.n, C.to_scipy()
            Cc = sp.coo_matrix((Cs.data.astype(np.float32), (np.repeat(np.arange(m),
                                np.diff(Cs.indptr)), Cs.indices)), shape=(m, m)).tocsr()
            Cc.sum_duplicates()
            C = DeviceCSR.from_scipy(sp.csr_matrix((Cc.data.astype(np.float64), Cc.indices,
                                                    Cc.indptr), shape=(m, m)), check=False)
        return C, bellman_ford_pyamg_device(C, seeds, fp64=fp64)[1]


# ----------------------------------------------------------------------------------- weights
class ModuleWeights:
    """Where a layer's run() takes its weights from: here the module's own parameters, one set
    shared by every member of the stack (pstride 0). Called with a parameter (or None), returns
    the tensor the kernel reads for member 0; member p's lies pstride floats further on."""
    pstride = 0

    def __call__(self, p):
        return None if p is None else p.detach().contiguous()


OWN = ModuleWeights()


class PopulationWeights(ModuleWeights):
    """The weights of a whole population for `model`'s layers: `population` is a (P, total)
    array of flat vectors in state_dict order (fitness.weights_as_vector's layout), uploaded once
    as one fp32 (P, total) tensor on the model's device (`data`; rounded like weights_as_dict's
    .to(float32)). Called with one of the model's parameters it returns member 0's tensor of it,
    a view into row 0; member p's lies pstride = total floats further on, which is how the *_pop
    kernels index it. view(name, member) is any member's tensor by state_dict name. The model's
    own parameters are neither read nor written."""

    def __init__(self, model, population):
        sd = model.state_dict()
        pop = np.asarray(population)
        total = sum(v.numel() for v in sd.values())
        if pop.ndim != 2 or pop.shape[0] < 1:
            raise ValueError("a population is a (P, total) array with P >= 1, got shape "
                             f"{pop.shape}")
        if pop.shape[1] != total:
            raise ValueError(f"weight vectors have {pop.shape[1]} entries, the model {total}")
        if any(v.dtype != torch.float32 for v in sd.values()):
            raise ValueError("a population stack takes a model whose tensors are all float32")
        dev = next(model.parameters()).device
        self.data = torch.as_tensor(np.ascontiguousarray(pop)).to(torch.float32).to(dev)
        self.members, self.pstride = int(pop.shape[0]), int(total)
        tensors = dict(model.named_parameters())
        tensors.update(model.named_buffers())
        self.layout, self._at, at = {}, {}, 0
        for name, v in sd.items():
            self.layout[name] = (at, tuple(v.shape))
            self._at[id(tensors[name])] = name
            at += v.numel()
        self._tensors = tensors  # kept alive: the ids above are theirs

    def view(self, name, member=0):
        at, shape = self.layout[name]
        return self.data[member, at:at + int(np.prod(shape, dtype=np.int64))].view(shape)

    def __call__(self, p):
        if p is None:
            return None
        if id(p) not in self._at:
            raise KeyError("not a parameter of the model this population was made for")
        return self.view(self._at[id(p)])

    def rows(self, a, b):
        """Members a .. b - 1 as a population of their own (views, nothing copied)."""
        w = object.__new__(type(self))
        w.__dict__.update(self.__dict__)
        w.data, w.members = self.data[a:b], b - a
        return w


# ------------------------------------------------------------------------------------ kernels
def linear(x, W, b=None, act=0, out=None, beta=0.0, residual=None, members=1, w=OWN):
    """members, w: the rows of x are `members` equal parts, part p on member p's W and b of the
    weight source w (OWN: W and b themselves, shared)."""
    x = x.contiguous()
    M, K = x.shape
    N = W.shape[0]
    if M % members:
        raise ValueError(f"{M} rows are not {members} equal parts")
    y = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=x.device)
    rc = 0 if residual is None else residual.shape[1]
    call("mlamg_gnn_linear_pop", ptr(x), int(M // members), int(members), int(K), ptr(w(W)),
         _p(w(b)), int(w.pstride), int(N), int(act), float(beta),
         _p(None if residual is None else residual.contiguous()), int(rc), ptr(y), stream_ptr())
    return y


def instance_norm(x, eps=1e-5):
    x = x.contiguous()
    y = torch.empty_like(x)
    call("mlamg_gnn_instance_norm", ptr(x), int(x.shape[0]), int(x.shape[1]), float(eps), ptr(y),
         stream_ptr())
    return y


def propagate(g, w, x):
    x = x.contiguous()
    y = torch.empty_like(x)
    call("mlamg_gnn_propagate", ptr(g.tptr), ptr(g.teid), ptr(g.src), ptr(w), ptr(x), int(g.n),
         int(x.shape[1]), ptr(y), stream_ptr())
    return y


def topk_vec(x, k):
    """agg_interp.py:14-22; ties broken by the smaller node index (torch.argsort leaves them
    unspecified)."""
    s = x.reshape(-1).contiguous()
    vec = torch.empty_like(s)
    idx = torch.empty(int(k), dtype=torch.int32, device=s.device)
    call("mlamg_gnn_topk", ptr(s), int(s.numel()), int(k), ptr(vec), _p(idx if k else None),
         stream_ptr())
    return vec, idx


def instance_norm_seg(x, seg, eps=1e-5):
    """instance_norm on every segment of a stack (seg: SegPtr of node offsets) in one launch;
    segment g is bitwise instance_norm(x[seg.host[g]:seg.host[g + 1]])."""
    x = x.contiguous()
    y = torch.empty_like(x)
    call("mlamg_gnn_instance_norm_seg", ptr(x), ptr(seg.dev), seg.host_ptr,
         seg.nb, int(x.shape[1]), float(eps), ptr(y), stream_ptr())
    return y


def topk_vec_seg(x, seg, kptr):
    """topk_vec on every segment of a stack: (vec, idx) with kptr.host[g + 1] - kptr.host[g]
    ones in segment g and their node ids in the stack, best first, in
    idx[kptr.host[g]:kptr.host[g + 1]]. Does not synchronise."""
    s = x.reshape(-1).contiguous()
    vec = torch.empty_like(s)
    idx = torch.empty(max(int(kptr.host[-1]), 1), dtype=torch.int32, device=s.device)
    call("mlamg_gnn_topk_seg", ptr(s), ptr(seg.dev), seg.host_ptr, ptr(kptr.dev), kptr.host_ptr,
         seg.nb, ptr(vec), ptr(idx), stream_ptr())
    return vec, idx[:int(kptr.host[-1])]


POPULATION_SCRATCH_BYTES = 2 << 30  # FullAggNet.members_per_pass: NNConv messages of one pass


def _join_passes(passes, stacks):
    """forward_stack's dicts of consecutive passes of a population as the dict of the whole
    stack: rows, aggregate columns and seed offsets of a pass shifted behind the earlier ones,
    every entry's own bits kept."""
    from .sparse import DeviceCSR
    rows = np.concatenate([[0], np.cumsum([s.n for s in stacks])])
    cols = np.concatenate([[0], np.cumsum([int(st["kptr"].host[-1]) for st in passes])])
    dev = stacks[0].device

    def offsets(ptrs, shifts):
        return np.concatenate([p.host[:-1] + s for p, s in zip(ptrs, shifts)]
                              + [[ptrs[-1].host[-1] + shifts[len(ptrs) - 1]]])

    def csr(key, coff):
        crows, cjs, vals, nnz = [], [], [], 0
        for i, st in enumerate(passes):
            crow, cj, v = st[key].to_torch()
            crows.append((crow if i == 0 else crow[1:]).long() + nnz)
            cjs.append(cj.long() + int(coff[i]))
            vals.append(v)
            nnz += int(st[key].nnz)
        return DeviceCSR.from_torch(torch.cat(crows).to(torch.int32),
                                    torch.cat(cjs).to(torch.int32), torch.cat(vals),
                                    (int(rows[-1]), int(coff[-1])))

    return dict(Agg=csr("Agg", cols), P=csr("P", cols), C=csr("C", rows),
                top_k=torch.cat([st["top_k"] + int(r) for st, r in zip(passes, rows)]),
                node_scores=torch.cat([st["node_scores"] for st in passes]),
                kptr=SegPtr(offsets([st["kptr"] for st in passes], cols), dev),
                seg=SegPtr(offsets([s.seg for s in stacks], rows), dev),
                failed=np.concatenate([np.asarray(st["failed"]).reshape(-1) for st in passes]))


# ------------------------------------------------------------------------------------ modules
class TensorLambda(nn.Module):
    """Parameter-free placeholder at index 0 of NNConv's edge network (agg_interp.py:24-34)."""

    def __init__(self, func=None):
        super().__init__()
        self.f = func

    def forward(self, x):
        return self.f(x) if self.f else x


class TAGConv(nn.Module):
    """torch_geometric TAGConv(in, out, K=3): sum_k lins[k](A_hat^k x) + bias."""

    def __init__(self, in_channels, out_channels, K=3):
        super().__init__()
        self.K = K
        self.lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False)
                                   for _ in range(K + 1)])
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def run(self, g, x, act=0, w=OWN):
        """w (here and in every layer below): the weight source, the module's own parameters or
        a PopulationWeights with one member per member of g."""
        wn = g.gcn_weights()
        out = linear(x, self.lins[0].weight, members=g.members, w=w)
        for k in range(1, self.K + 1):
            x = propagate(g, wn, x)
            last = k == self.K
            out = linear(x, self.lins[k].weight, b=self.bias if last else None,
                         act=act if last else 0, out=out, beta=1.0, members=g.members, w=w)
        return out


class NNConv(nn.Module):
    """torch_geometric NNConv(in, out, nn, aggr='add'): sum over incoming edges of
    x_src @ nn(e).view(in, out), + lin(x) (root weight), + bias."""

    def __init__(self, in_channels, out_channels, edge_features):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.nn = nn.Sequential(TensorLambda(), nn.Linear(edge_features, 4), nn.ReLU(),
                                nn.Linear(4, 16), nn.ReLU(),
                                nn.Linear(16, in_channels * out_channels), nn.ReLU())
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def run(self, g, x, ea, act=0, residual=None, w=OWN):
        x = x.contiguous()
        ea = ea.contiguous()
        n = x.shape[0]
        root = linear(x, self.lin.weight, members=g.members, w=w)
        msg = torch.empty((max(g.E, 1), self.out_channels), dtype=torch.float32, device=x.device)
        y = torch.empty((n, self.out_channels), dtype=torch.float32, device=x.device)
        L1, L2, L3 = self.nn[1], self.nn[3], self.nn[5]
        rc = 0 if residual is None else residual.shape[1]
        call("mlamg_gnn_nnconv_pop", ptr(g.tptr), ptr(g.teid), ptr(g.src), ptr(ea),
             int(g.member_E), int(g.members), int(ea.shape[1]), ptr(w(L1.weight)),
             ptr(w(L1.bias)), ptr(w(L2.weight)), ptr(w(L2.bias)), ptr(w(L3.weight)),
             ptr(w(L3.bias)), int(w.pstride), ptr(x), int(n // g.members),
             int(self.in_channels), int(self.out_channels), ptr(root), ptr(w(self.bias)),
             int(act), _p(None if residual is None else residual.contiguous()), int(rc),
             ptr(msg), ptr(y), stream_ptr())
        return y


class SmallEdgeModel(nn.Module):
    """agg_interp.py:37-55: Linear(in, hid) - ReLU - LayerNorm - Linear(hid, out)."""

    def __init__(self, in_dim, hid_dim, out_dim):
        super().__init__()
        self.edge_mlp = nn.Sequential(nn.Linear(in_dim, hid_dim), nn.ReLU(),
                                      nn.LayerNorm([hid_dim]), nn.Linear(hid_dim, out_dim))

    def run(self, g, x, ea, act=0, residual=None, w=OWN):
        l1, ln, l2 = self.edge_mlp[0], self.edge_mlp[2], self.edge_mlp[3]
        x = x.contiguous()
        ea = ea.contiguous()
        C = l2.weight.shape[0]
        out = torch.empty((max(g.E, 1), C), dtype=torch.float32, device=x.device)
        rc = 0 if residual is None else residual.shape[1]
        call("mlamg_gnn_edge_mlp_pop", ptr(g.src), ptr(g.tgt), ptr(x), int(x.shape[1]), ptr(ea),
             int(ea.shape[1]), int(g.member_E), int(g.members), ptr(w(l1.weight)),
             ptr(w(l1.bias)), int(l1.weight.shape[0]), ptr(w(ln.weight)), ptr(w(ln.bias)),
             ptr(w(l2.weight)), ptr(w(l2.bias)), int(w.pstride), int(C), int(act),
             _p(None if residual is None else residual.contiguous()), int(rc), ptr(out),
             stream_ptr())
        return out[:g.E]


class MPNN(nn.Module):
    """agg_interp.py:80-141 (node/edge activations ReLU)."""

    def __init__(self, dim, num_internal_conv=4, input_edge_features=1):
        super().__init__()
        self.node_conv_in = NNConv(1, dim, input_edge_features)
        self.normalize_in = nn.Identity()  # InstanceNorm(dim): no parameters
        self.edge_conv_in = SmallEdgeModel(dim * 2 + input_edge_features, dim, 2)
        self.node_convs = nn.ModuleList([NNConv(dim, dim, 2) for _ in range(num_internal_conv)])
        self.edge_convs = nn.ModuleList([SmallEdgeModel(dim * 2 + 2, dim, 2)
                                         for _ in range(num_internal_conv)])
        self.normalizations = nn.ModuleList([nn.Identity() for _ in range(num_internal_conv)])
        self.num_internal_conv = num_internal_conv
        self.node_conv_out = NNConv(dim, 1, 2)
        self.normalize_out = nn.Identity()
        self.edge_conv_out = SmallEdgeModel(4, dim, 1)

    @torch.no_grad()
    def run(self, g, w=OWN):
        x = g.x
        ea = g.edge_attr
        x = self.node_conv_in.run(g, instance_norm_seg(x, g.seg), ea, act=1, residual=x, w=w)
        ea = self.edge_conv_in.run(g, x, ea, act=1, residual=ea, w=w)
        for i in range(self.num_internal_conv):
            x = self.node_convs[i].run(g, instance_norm_seg(x, g.seg), ea, act=1, residual=x,
                                       w=w)
            ea = self.edge_convs[i].run(g, x, ea, act=1, residual=ea, w=w)
        x = self.node_conv_out.run(g, instance_norm_seg(x, g.seg), ea, act=1, w=w)
        ea = self.edge_conv_out.run(g, x, ea, act=1, w=w)
        return x, ea


def _fc(dim, last_out):
    layers = []
    for i in range(5 if last_out is None else 4):
        layers += [nn.Linear(dim, dim), nn.ReLU()]
    if last_out is not None:
        layers += [nn.Linear(dim, last_out), nn.ReLU()]
    return nn.Sequential(*layers)


class AggBinarizationLayer(nn.Module):
    """agg_interp.py:144-220."""

    def __init__(self, dim, num_conv=6):
        super().__init__()
        ncs = [TAGConv(1, dim)] + [TAGConv(dim, dim) for _ in range(num_conv - 1)]
        fcs = [_fc(dim, None) for _ in range(num_conv - 1)] + [_fc(dim, 1)]
        self.ncs = nn.ModuleList(ncs)
        self.fcs = nn.ModuleList(fcs)
        self.norms = nn.ModuleList([nn.Identity() for _ in range(num_conv)])  # InstanceNorm
        self.num_conv = num_conv
        self.dim = dim

    def run_raw(self, g, x, w=OWN):
        if x.dim() == 1:
            x = x.unsqueeze(1)
        for i in range(self.num_conv):
            x = instance_norm_seg(x, g.seg)
            x = self.ncs[i].run(g, x, act=1, w=w)   # relu(TAGConv(x))
            for lin in self.fcs[i]:
                if isinstance(lin, nn.Linear):
                    x = linear(x, lin.weight, lin.bias, act=1, members=g.members, w=w)
        return x

    @torch.no_grad()
    def run(self, g, x, k, w=OWN):
        """k: the seed offsets per graph (SegPtr); one graph alone also takes its seed count."""
        return topk_vec_seg(self.run_raw(g, x, w), g.seg, g.seed_ptr(k))[0]


class AggNet(nn.Module):
    """agg_interp.py:223-241."""

    def __init__(self, dim, iterations=2, num_conv=6):
        super().__init__()
        self.layers = nn.ModuleList([AggBinarizationLayer(dim, num_conv=num_conv)
                                     for _ in range(iterations)])
        self.num_iterations = iterations

    @torch.no_grad()
    def run(self, g, k, w=OWN):
        x = g.x
        for layer in self.layers:
            x = layer.run(g, x, k, w)
        return x


class FullAggNet(nn.Module):
    """agg_interp.py:379-486 (inference)."""

    def __init__(self, dim=64, num_conv=2, iterations=4):
        super().__init__()
        self.PNet = MPNN(dim, num_internal_conv=4, input_edge_features=2)
        self.AggNet = AggNet(dim, num_conv=num_conv, iterations=iterations)
        self.CNet = MPNN(dim, num_internal_conv=5)

    @property
    def device(self):
        return next(self.parameters()).device

    @torch.no_grad()
    def forward(self, A, alpha, aggregation="pyamg", x=None):
        """Returns (agg, P, bf_weights, cluster_centers, node_weights) like :442-486: agg and P
        as torch sparse COO (n x k, fp32), bf_weights as torch sparse COO (the CNet edge
        values C, edge (i, j) = A's entry (i, j)), cluster_centers the seed nodes (ascending),
        node_weights the 0/1 scores.

        aggregation: "pyamg" (default) is the reference's step, pyamg.graph.bellman_ford(C,
        top_k) (:475): pull sweeps x_i <- min(x_i, C_ij + x_j) in float32, emulated exactly
        on the device (graph.bellman_ford_pyamg_device), so every node's nearest seed is pyamg's,
        ties included; a node no seed reaches raises KeyError like nearest_center_to_agg's dict
        lookup (ns/lib/graph.py:83). "parallel" runs the same distances with the multi-workgroup
        order-independent Bellman-Ford (graph.hip k_bf_sweep, on C^T so the direction is
        pyamg's): nearest seeds equal pyamg's whenever shortest paths are unique, ties go to the
        smallest seed id, unreached nodes get no aggregate. "pyamg64": pyamg's sweeps in float64
        on the widened weights (what a pyamg build binding only double computes; the pyamg
        version is unpinned). x: node features replacing the
        reference graph's constant 1/n (graph_from_matrix_basic, ns/model/data.py:22-31) —
        not in the reference's signature; a test hook for well-conditioned inputs."""
        st = self.forward_stack(Graph(A, device=self.device), alpha, aggregation, x, strict=True)

        def to_t(M, dtype=torch.float32):
            crow, cj, v = M.to_torch()
            rows = torch.repeat_interleave(torch.arange(M.shape[0], device=crow.device),
                                           (crow[1:] - crow[:-1]).long())
            return torch.sparse_coo_tensor(torch.stack([rows, cj.long()]), v.to(dtype),
                                           M.shape).coalesce()

        return (to_t(st["Agg"]), to_t(st["P"]), to_t(st["C"]), st["top_k"], st["node_scores"])

    @torch.no_grad()
    def forward_stack(self, batch, alpha, aggregation="pyamg", x=None, strict=False,
                      weights=None):
        """The forward pass (:442-486) on every graph of `batch`, a GraphBatch or a Graph (a
        batch of one; nothing else is accepted), at once, results still stacked: a dict with
        Agg, P, C (DeviceCSR on stack rows; Agg and P on stacked aggregate columns; C as pyamg
        swept it), top_k (seed node ids in the
        stack, ascending), node_scores, kptr (SegPtr: seed / column offsets per graph) and failed
        (numpy bool per graph: some node reached by no seed; "parallel" never fails; strict:
        KeyError(-1) instead, before PNet runs). Every step is one call on the stack, so
        launches and host synchronisations do not depend on the batch size, and every graph's
        part carries the bits it has when the graph runs alone. weights: a PopulationWeights
        with one member per member of a PopulationBatch, instead of the model's own parameters
        (forward_population)."""
        from .graph import aggregate_op_device, bellman_ford_device, labels_to_columns
        if aggregation not in ("pyamg", "pyamg64", "parallel"):
            raise ValueError("aggregation must be 'pyamg', 'pyamg64' or 'parallel', got "
                             f"{aggregation!r}")
        w = OWN if weights is None else weights
        if weights is not None and weights.members != batch.members:
            raise ValueError(f"{weights.members} weight sets for a stack of {batch.members} "
                             "members")
        g = batch if x is None else batch.with_x(x)
        kptr = batch.k_ptr(alpha)
        node_scores = self.AggNet.run(g, kptr, w).reshape(-1)
        top_k = torch.nonzero(node_scores == 1).reshape(-1)  # k_g per graph, graph after graph
        # Bellman-Ford over the CNet edge weights from the seeds (:466-475), on the device
        _, bf_edges = self.CNet.run(g, w)
        C = g.csr(bf_edges)
        seeds = top_k.to(torch.int32)
        failed = np.zeros(batch.nb, dtype=bool)
        if aggregation != "parallel":
            C, lab = batch.pyamg_sweep(C, seeds, kptr, aggregation == "pyamg64")
            if batch.nb == 1:  # one reduction instead of the count per graph
                failed = np.array([bool((lab < 0).any())])
            else:
                lost = torch.zeros(batch.nb, dtype=torch.int32, device=lab.device)
                lost.index_add_(0, batch.node_gid, (lab < 0).to(torch.int32))
                failed = lost.cpu().numpy() > 0
            if strict and failed.any():
                raise KeyError(-1)
        else:
            _, lab, _ = bellman_ford_device(C.T, seeds)
        col = labels_to_columns(lab, seeds)
        Agg = aggregate_op_device(col, int(kptr.host[-1]))
        # P_hat from PNet on graph_from_matrix(A, Agg), P = P_hat Agg (:476-484)
        _, p_edges = self.PNet.run(g.with_clusters(col), w)
        P = g.csr(p_edges) @ Agg
        return dict(Agg=Agg, P=P, C=C, top_k=top_k, node_scores=node_scores, kptr=kptr,
                    failed=failed)

    def members_per_pass(self, batch):
        """The default split of forward_population: the largest number of members whose stack
        of `batch` stays inside the kernels' limits (65535 members, fewer than 2^31 - 1 rows
        and edges) and whose NNConv messages, members * E * dim * 4 bytes — the dominant
        scratch term of a pass — stay inside POPULATION_SCRATCH_BYTES (2 GiB)."""
        dim = self.AggNet.layers[0].dim
        by_index = (2 ** 31 - 2) // max(batch.n, batch.E, 1)
        by_scratch = POPULATION_SCRATCH_BYTES // max(batch.E * dim * 4, 1)
        return int(max(1, min(65535, by_index, by_scratch)))

    @torch.no_grad()
    def forward_population(self, batch, population, alpha, aggregation="pyamg", x=None,
                           members_per_pass=None):
        """forward_stack for every individual of a population at once: `population` is a
        (P, total) array of flat weight vectors in state_dict order (or a PopulationWeights made
        from one), `batch` the GraphBatch of nb graphs they are all scored on. Returns
        forward_stack's dict for the stack of P x nb graphs, member-major (member p's graph g
        is segment p nb + g: rows, aggregate columns, top_k and kptr all run over that stack),
        with `failed` of shape (P, nb) and `seg`, the stack's node offsets (SegPtr). Member p's
        part is bitwise forward_stack(batch, ...) after load_state_dict(weights_as_dict(model,
        population[p])); the model's own parameters are neither read nor written.

        The stack is batch.population(m) (a PopulationBatch, cached on the batch with its
        Bellman-Ford plan); the three weight-consuming kernels take member p's tensors from row p
        of the population (mlamg_gnn_*_pop), every other step sees P x nb segments.
        members_per_pass splits the population into consecutive passes of that many members (the
        last may be shorter), whose results are joined; the default is self.members_per_pass(
        batch). The results do not depend on the split; the joined stack itself must fit int32
        row and entry counts. Whether one pass is faster than P forward_stack calls is
        unmeasured (tools/bench_gnn_population.py is the benchmark). x: the
        per-node input hook of forward(), for the nb graphs (every member gets the same)."""
        pw = population if isinstance(population, PopulationWeights) \
            else PopulationWeights(self, population)
        P = pw.members
        chunk = int(members_per_pass) if members_per_pass else self.members_per_pass(batch)
        if chunk < 1:
            raise ValueError("members_per_pass must be at least 1")
        if x is not None:
            x = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x,
                                dtype=torch.float32).reshape(-1)
        passes, stacks = [], []
        for a in range(0, P, chunk):
            m = min(chunk, P - a)
            pb = batch.population(m)
            stacks.append(pb)
            passes.append(self.forward_stack(pb, alpha, aggregation,
                                             None if x is None else x.repeat(m),
                                             weights=pw.rows(a, a + m)))
        st = passes[0] if len(passes) == 1 else _join_passes(passes, stacks)
        if len(passes) == 1:
            st["seg"] = stacks[0].seg
        st["failed"] = st["failed"].reshape(P, batch.nb)
        return st

    @torch.no_grad()
    def forward_batch(self, batch, alpha, aggregation="pyamg", x=None, strict=False):
        """forward(A_g, alpha, aggregation) for every graph g of a GraphBatch, in a fixed
        number of launches: a list with one entry per graph, the tuple forward() returns (local
        indices, same dtypes, bitwise the same tensors) or None for a graph in which some node
        is reached by no seed (forward() raises KeyError(-1) there; strict=True raises KeyError
        naming the first such graph). The other graphs' results do not depend on a failed one.
        k_g = ceil(alpha n_g). x: the per-node input hook of forward(), the graphs' inputs
        concatenated. The sparse tensors of an entry are views into the stacked results."""
        st = self.forward_stack(batch, alpha, aggregation, x)
        failed, kptr = st["failed"], st["kptr"]
        if strict and failed.any():
            raise KeyError(f"graph {int(np.argmax(failed))} of the batch: a node is reached by "
                           "no seed (-1)")
        seg, gid = batch.seg, batch.node_gid
        nrow = torch.arange(batch.n, device=gid.device)

        def stacked(M, coff, sort=False):
            """(crow, local COO indices [2, nnz], fp32 values) of a stacked DeviceCSR, rows in
            order and (sort: the SpGEMM leaves scipy's column order) columns ascending, as
            forward()'s coalesce() leaves them."""
            crow, cj, v = M.to_torch()
            rows = torch.repeat_interleave(nrow, (crow[1:] - crow[:-1]).long(),
                                           output_size=M.nnz)
            cj = cj.long()
            if sort:
                order = torch.argsort(rows * M.shape[1] + cj)  # unique keys: one order
                cj, v = cj[order], v[order]
            gr = gid[rows]
            return crow, torch.stack([rows - seg.dev[gr], cj - coff[gr]]), v.to(torch.float32)

        crow_a, idx_a, val_a = stacked(st["Agg"], kptr.dev)
        crow_p, idx_p, val_p = stacked(st["P"], kptr.dev, sort=True)
        _, idx_c, val_c = stacked(st["C"], seg.dev)
        cuts = torch.stack([crow_a[seg.dev], crow_p[seg.dev]]).cpu().numpy()
        top_k = st["top_k"]
        top_local = top_k - seg.dev[gid[top_k]]

        def coo(idx, val, a, b, shape):
            return torch.sparse_coo_tensor(idx[:, a:b], val[a:b], shape, is_coalesced=True)

        out = []
        for i in range(batch.nb):
            if failed[i]:
                out.append(None)
                continue
            n = int(batch.sizes[i])
            k0, k1 = int(kptr.host[i]), int(kptr.host[i + 1])
            r0, e0, e1 = int(seg.host[i]), int(batch.eseg.host[i]), int(batch.eseg.host[i + 1])
            out.append((coo(idx_a, val_a, int(cuts[0, i]), int(cuts[0, i + 1]), (n, k1 - k0)),
                        coo(idx_p, val_p, int(cuts[1, i]), int(cuts[1, i + 1]), (n, k1 - k0)),
                        coo(idx_c, val_c, e0, e1, (n, n)),
                        top_local[k0:k1], st["node_scores"][r0:r0 + n]))
        return out
