"""The learned interpolation of the reference preconditioner on the device.

Mirrors ns/model/ali_interp.py: `InterpolationNetwork.forward_mat(A, C, F)` (:283-285) builds the
C/F graph of A, runs `ResidualBlock(1, 1, 9, [16, 16, 32, 32, 64, 64, 128, 128, 256, 256], K=5)`
(20 TAGConv layers of 5 hops, then an EdgeModel 513 -> 256 -> ... -> 16 -> 1 with LayerNorms) and
assembles P from the edge values. It is step 2 of ns/preconditioner/MLAMG.py's setup (:105-120),
after the greedy C/F splitting (mlamg.greedy).

The forward pass runs on HIP kernels, fp32 like the reference: layers up to 64 channels on
csrc/gnn.hip, wider ones on csrc/gnn_wide.hip (dense products on the f32-input matrix cores, the
first EdgeModel block without its E x 513 concatenation). DESIGN.md §31.

Parameter names. The modules hold their parameters under the reference's names where its source
fixes them: `edge_model.blocks.{i}.{j}`, `edge_model.network.{j}` (the same Linear modules,
registered twice like the reference's) and `edge_model.normaliz.{i}`. The TAGConv layers live in
a torch_geometric `Sequential` there; its children are named `module_{i}` in PyG 2.x, giving
`network.module_{i}.lins.{k}.weight` and `network.module_{i}.bias` with the TAGConvs at positions
0, 1 + 3i, 3 + 3i (i = 0..8) and 28. torch_geometric is absent here, so these key names are
UNVERIFIED against a real reference checkpoint. The reference loads the state_dict into
`InterpolationNetwork.model` (MLAMG.py:108), so the keys above are those of `ResidualBlock`.

Stated differences: torch_geometric's layers (TAGConv with gcn_norm and no self loops,
InstanceNorm without affine parameters) are restated from its 2.x semantics and parity with it is
unpinned (tests/interp_ref.py is the plain-torch restatement the device is held to); the edges run
in A's row-major order, not networkx's; explicit zeros the network produces stay stored in P;
P's values are fp32 numbers carried in an fp64 CSR.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn

from . import gnn
from ._lib import call, ptr, stream_ptr
from .gnn import _p

DIMS = (16, 16, 32, 32, 64, 64, 128, 128, 256, 256)
HOPS = 5
LN_EPS = 1e-5
NARROW_K, NARROW_N, NARROW_F = 160, 64, 64  # the limits of csrc/gnn.hip's kernels


# ------------------------------------------------------------------------------------ kernels
def linear_wide(x, W, b=None, act=0, out=None, beta=0.0, residual=None):
    """gnn.linear's contract on mlamg_gnn_linear_wide (K <= 1024, N <= 256)."""
    x = x.contiguous()
    M, K = x.shape
    N = W.shape[0]
    y = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=x.device)
    rc = 0 if residual is None else residual.shape[1]
    # contiguous copies stay in variables until the launch: a temporary's block could be handed
    # to the next copy before the kernel has read it
    W = W.detach().contiguous()
    b = None if b is None else b.detach().contiguous()
    residual = None if residual is None else residual.contiguous()
    call("mlamg_gnn_linear_wide", ptr(x), int(M), int(K), ptr(W), _p(b), int(N), int(act),
         float(beta), _p(residual), int(rc), ptr(y), stream_ptr())
    return y


def linear(x, W, b=None, act=0, out=None, beta=0.0, residual=None):
    """The narrow kernel where it accepts the shape, the wide one beyond."""
    f = gnn.linear if W.shape[1] <= NARROW_K and W.shape[0] <= NARROW_N else linear_wide
    return f(x, W, b=b, act=act, out=out, beta=beta, residual=residual)


def propagate(g, w, x):
    x = x.contiguous()
    if x.shape[1] <= NARROW_F:
        return gnn.propagate(g, w, x)
    y = torch.empty_like(x)
    call("mlamg_gnn_propagate_wide", ptr(g.tptr), ptr(g.teid), ptr(g.src), ptr(w), ptr(x),
         int(g.n), int(x.shape[1]), ptr(y), stream_ptr())
    return y


def layer_norm(x, weight=None, bias=None, eps=LN_EPS, residual=None, act=0):
    """act(LayerNorm(x) * weight + bias + residual) over rows of up to 256 features."""
    x = x.contiguous()
    y = torch.empty_like(x)
    weight = None if weight is None else weight.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    residual = None if residual is None else residual.contiguous()
    call("mlamg_gnn_layer_norm", ptr(x), int(x.shape[0]), int(x.shape[1]), _p(weight), _p(bias),
         float(eps), _p(residual), int(act), ptr(y), stream_ptr())
    return y


def edge_in(g, U, V, ea, w, b, ln_weight, ln_bias, eps=LN_EPS):
    """relu(LayerNorm((U[src] + V[tgt]) + ea w + b)) per edge: the first EdgeModel block from
    the two node products."""
    H = U.shape[1]
    out = torch.empty((g.E, H), dtype=torch.float32, device=U.device)
    U, V, ea = U.contiguous(), V.contiguous(), ea.reshape(-1).contiguous()
    w, b, lw, lb = (t.detach().contiguous() for t in (w, b, ln_weight, ln_bias))
    call("mlamg_gnn_edge_in", ptr(g.src), ptr(g.tgt), ptr(U), ptr(V), ptr(ea), int(g.E), int(H),
         ptr(w), ptr(b), ptr(lw), ptr(lb), float(eps), ptr(out), stream_ptr())
    return out


def standardize_abs(v):
    """|(v - mean) / std| with torch's unbiased std (ali_interp.py:174-175)."""
    v = v.contiguous()
    out = torch.empty_like(v)
    call("mlamg_gnn_standardize_abs", ptr(v), int(v.numel()), ptr(out), stream_ptr())
    return out


def tag_conv(conv, g, x, act=0):
    """gnn.TAGConv.run with the kernel chosen by width: sum_k lins[k](A_hat^k x) + bias."""
    wn = g.gcn_weights()
    out = linear(x, conv.lins[0].weight)
    for k in range(1, conv.K + 1):
        x = propagate(g, wn, x)
        last = k == conv.K
        out = linear(x, conv.lins[k].weight, b=conv.bias if last else None,
                     act=act if last else 0, out=out, beta=1.0)
    return out


# ------------------------------------------------------------------------------------ modules
class EdgeModel(nn.Module):
    """ali_interp.py:49-104: Linear blocks with a LayerNorm each, residual add where shapes
    agree, ReLU; the last block is a bare Linear."""

    def __init__(self, in_dim, dims, out_dim):
        super().__init__()
        blocks, norms, params = [], [], []
        first = [nn.Linear(in_dim, dims[0])]
        params += first
        blocks.append(nn.Sequential(*first))
        norms.append(nn.LayerNorm(dims[0]))
        for i in range(len(dims) - 1):
            blk = [nn.Linear(dims[i], dims[i + 1]), nn.ReLU(), nn.Linear(dims[i + 1], dims[i + 1])]
            params += blk
            blocks.append(nn.Sequential(*blk))
            norms.append(nn.LayerNorm(dims[i + 1]))
        last = [nn.Linear(dims[-1], out_dim)]
        params += last
        blocks.append(nn.Sequential(*last))
        norms.append(nn.Identity())
        self.blocks = nn.ModuleList(blocks)
        self.normaliz = nn.ModuleList(norms)
        self.network = nn.Sequential(*params)  # the same modules again, as in the reference
        self.n_blocks = len(blocks)

    def layer(self, i, g, x):
        """Block i on the device. Block 0 takes the node features (n x F) and gathers them per
        edge itself; the others take the previous block's edge features."""
        if i == 0:
            lin, ln = self.blocks[0][0], self.normaliz[0]
            F = x.shape[1]
            W = lin.weight.detach()
            U = linear(x, W[:, :F].contiguous())
            V = linear(x, W[:, F:2 * F].contiguous())
            return edge_in(g, U, V, g.edge_attr[:, 0], W[:, 2 * F].contiguous(), lin.bias,
                           ln.weight, ln.bias, ln.eps)
        if i == self.n_blocks - 1:
            lin = self.blocks[i][0]
            return linear(x, lin.weight, lin.bias)
        l1, l2, ln = self.blocks[i][0], self.blocks[i][2], self.normaliz[i]
        y = linear(linear(x, l1.weight, l1.bias, act=1), l2.weight, l2.bias)
        same = l2.weight.shape[0] == x.shape[1]
        return layer_norm(y, ln.weight, ln.bias, ln.eps, residual=x if same else None, act=1)

    def run(self, g, x):
        for i in range(self.n_blocks):
            x = self.layer(i, g, x)
        return x


class ResidualBlock(nn.Module):
    """ali_interp.py:107-175 (inference): TAGConv blocks with InstanceNorm after every block but
    the last, residual add where shapes agree, ReLU; then the EdgeModel on [x_src | x_tgt | ea]
    and |standardised| edge values."""

    def __init__(self, in_channels=1, out_channels=1, res_layers=9, dim=DIMS, K=HOPS):
        super().__init__()
        self.in_channels, self.out_channels, self.res_layers, self.dim, self.K = \
            in_channels, out_channels, res_layers, tuple(dim), K
        seq = [gnn.TAGConv(in_channels, dim[0], K=K)]
        self._blocks = [(0,)]  # positions of each block's TAGConvs in `network`
        for i in range(res_layers):
            self._blocks.append((len(seq), len(seq) + 2))
            seq += [gnn.TAGConv(dim[i], dim[i + 1], K=K), nn.ReLU(),
                    gnn.TAGConv(dim[i + 1], dim[i + 1], K=K)]
        self._blocks.append((len(seq),))
        seq.append(gnn.TAGConv(dim[-1], dim[-1], K=K))
        self.network = nn.Module()  # torch_geometric.nn.Sequential's child names
        for j, m in enumerate(seq):
            self.network.add_module(f"module_{j}", m)
        self._seq = seq
        self.edge_model = EdgeModel(dim[-1] * 2 + 1, tuple(dim[::-1]), 1)
        self.n_blocks = len(self._blocks)

    def node_layer(self, i, g, x):
        """Block i on the device: conv (ReLU conv), InstanceNorm (not after the last block),
        + input where shapes agree, ReLU."""
        pos = self._blocks[i]
        y = tag_conv(self._seq[pos[0]], g, x, act=1 if len(pos) == 2 else 0)
        if len(pos) == 2:
            y = tag_conv(self._seq[pos[1]], g, y)
        if i != self.n_blocks - 1:
            y = gnn.instance_norm(y)
        if y.shape == x.shape:
            y = y + x
        return torch.relu_(y)

    def run_nodes(self, g):
        x = g.x
        for i in range(self.n_blocks):
            x = self.node_layer(i, g, x)
        return x

    @torch.no_grad()
    def run(self, g):
        """The E x 1 edge values of forward(D) (:151-175)."""
        return standardize_abs(self.edge_model.run(g, self.run_nodes(g)))


def graph_from_matrix(A, C, F, device=None):
    """ali_interp.py:235-256 as a gnn.Graph: the edges are the stored entries (i, j) of A with
    exactly one end in C (the C-C and F-F edges, self loops among them, are removed), in row-major
    order; edge_attr = |a_ij|, x = the indicator of C. ValueError unless A is symmetric (the
    reference's undirected networkx graph would keep one of the two values) and C, F split the
    rows."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"graph_from_matrix needs a square matrix, got {A.shape}")
    if (A != A.T).nnz != 0:
        raise ValueError("graph_from_matrix needs a symmetric matrix")
    C, F = np.asarray(C, dtype=np.int64).ravel(), np.asarray(F, dtype=np.int64).ravel()
    is_c = np.zeros(n, dtype=bool)
    is_c[C] = True
    if len(C) + len(F) != n or is_c.sum() != len(C) or is_c[F].any():
        raise ValueError("C and F must split the rows of A")
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    keep = is_c[rows] != is_c[A.indices]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=indptr[1:])
    A_cf = sp.csr_matrix((A.data[keep], A.indices[keep], indptr), shape=A.shape)
    return gnn.Graph(A_cf, device=device).with_x(is_c.astype(np.float32))


def assemble_P(n, src, tgt, vals, C):
    """The rule of forward() (:258-281) in device-agnostic torch: an n x n matrix of the edge
    values, ones on the diagonal at C, the columns C in C's order. -> (indptr, indices, data) of
    the n x len(C) CSR (int64, int64, float64), columns ascending within a row like scipy's
    tocsc()[:, C].tocsr(). The edges must be duplicate-free."""
    dev = vals.device
    C = torch.as_tensor(C, dtype=torch.int64, device=dev)
    src, tgt = src.to(torch.int64), tgt.to(torch.int64)
    nc = C.numel()
    col_of = torch.full((n,), -1, dtype=torch.int64, device=dev)
    col_of[C] = torch.arange(nc, dtype=torch.int64, device=dev)
    keep = (col_of[tgt] >= 0) & (src != tgt)
    rows = torch.cat([src[keep], C])
    cols = torch.cat([col_of[tgt[keep]], torch.arange(nc, dtype=torch.int64, device=dev)])
    data = torch.cat([vals.reshape(-1)[keep].to(torch.float64),
                      torch.ones(nc, dtype=torch.float64, device=dev)])
    order = torch.argsort(rows * max(nc, 1) + cols)  # unique keys: one order
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return indptr, cols[order], data[order]


class InterpolationNetwork(nn.Module):
    """ali_interp.py:228-285 (inference). `model` is the ResidualBlock the reference's
    preconditioner loads its state_dict into."""

    def __init__(self):
        super().__init__()
        self.hops = HOPS
        self.model = ResidualBlock(1, 1, 9, DIMS, self.hops)

    @property
    def device(self):
        return next(self.parameters()).device

    def graph_from_matrix(self, A, C, F):
        return graph_from_matrix(A, C, F, device=self.device)

    @torch.no_grad()
    def forward(self, G, A, C, F):
        n = A.shape[1]
        if G.E < 2:
            raise ValueError("the C/F graph has fewer than two edges: the standardisation of the "
                             "edge values (ali_interp.py:174) is undefined")
        vals = self.model.run(G)
        indptr, indices, data = assemble_P(n, G.src, G.tgt, vals, C)
        return sp.csr_matrix((data.cpu().numpy(), indices.cpu().numpy().astype(np.int32),
                              indptr.cpu().numpy().astype(np.int32)), shape=(n, len(C)))

    def forward_mat(self, A, C, F):
        """P (scipy CSR, n x len(C)) for the splitting C, F of A."""
        return self.forward(self.graph_from_matrix(A, C, F), A, C, F)
