"""Plain-torch restatement of ns/model/ali_interp.py's ResidualBlock / EdgeModel / forward on the
CPU, parametrised by dtype: the yardstick of mlamg.interp (tests/test_interp_host.py validates it,
tests/test_gpu_interp.py holds the device to it). It reads a state_dict under the key names
mlamg/interp.py documents and works on an edge list (src, tgt, |a|) in any order, with
torch_geometric 2.x's semantics written out: TAGConv(K, normalize=True) = sum_k lins[k](A_hat^k x)
+ bias on gcn_norm weights without self loops, InstanceNorm without affine parameters (biased
variance, eps 1e-5), torch LayerNorm, torch.std unbiased.

reverse=True evaluates every dense product, LayerNorm sum and aggregation in the opposite order
(features reversed, edges reversed): a second legitimate floating-point order of the same
function, used to measure how far two correct fp32 evaluations lie apart."""
import numpy as np
import torch

DIMS = (16, 16, 32, 32, 64, 64, 128, 128, 256, 256)
HOPS = 5
EPS = 1e-5
# positions of each node block's TAGConvs in `network`, and of each edge block's Linears
NODE_BLOCKS = [(0,)] + [(1 + 3 * i, 3 + 3 * i) for i in range(9)] + [(28,)]
N_EDGE_BLOCKS = 11


class Ref:
    def __init__(self, state_dict, src, tgt, ea, dtype, reverse=False, device="cpu"):
        """src, tgt, ea: numpy arrays. device: where the restatement runs (the tests use the CPU;
        tools/interp_timing.py times it on the GPU as the plain-torch baseline)."""
        self.dt = dtype
        self.rev = reverse
        self.dev = torch.device(device)
        self.sd = {k: v.detach().to(self.dev, dtype) for k, v in state_dict.items()}
        self.src = torch.as_tensor(np.asarray(src), dtype=torch.int64).to(self.dev)
        self.tgt = torch.as_tensor(np.asarray(tgt), dtype=torch.int64).to(self.dev)
        self.ea = torch.as_tensor(np.asarray(ea)).reshape(-1).to(torch.float32).to(self.dev, dtype)
        self.order = torch.arange(len(self.src), device=self.dev)
        if reverse:
            self.order = self.order.flip(0)

    def t(self, x):
        if isinstance(x, torch.Tensor):
            return x.to(self.dev, self.dt)
        return torch.as_tensor(np.asarray(x)).to(self.dev, self.dt)

    # ------------------------------------------------------------------ pieces
    def lin(self, x, W, b=None):
        y = x.flip(1) @ W.flip(1).T if self.rev else x @ W.T
        return y if b is None else y + b

    def gcn_weights(self, n):
        deg = torch.zeros(n, dtype=self.dt, device=self.dev).index_add_(0, self.tgt[self.order],
                                                       self.ea[self.order])
        dis = deg.pow(-0.5)
        dis[torch.isinf(dis)] = 0
        return dis[self.src] * self.ea * dis[self.tgt]

    def propagate(self, wn, x):
        o = self.order
        return torch.zeros_like(x).index_add_(0, self.tgt[o], wn[o, None] * x[self.src[o]])

    def tag(self, pos, x, wn):
        p = f"network.module_{pos}."
        out = self.lin(x, self.sd[p + "lins.0.weight"])
        for k in range(1, HOPS + 1):
            x = self.propagate(wn, x)
            out = out + self.lin(x, self.sd[p + f"lins.{k}.weight"])
        return out + self.sd[p + "bias"]

    def inorm(self, x):
        mean = x.mean(0, keepdim=True)
        var = ((x - mean) ** 2).mean(0, keepdim=True)
        return (x - mean) / torch.sqrt(var + EPS)

    def lnorm(self, x, w, b):
        xs = x.flip(1) if self.rev else x
        mean = xs.mean(1, keepdim=True)
        var = ((xs - mean) ** 2).mean(1, keepdim=True)
        return (x - mean) / torch.sqrt(var + EPS) * w + b

    # ------------------------------------------------------------------ layers
    def node_layer(self, i, x):
        """Block i of ResidualBlock.forward's loop on node features x (n x channels)."""
        x = self.t(x)
        wn = self.gcn_weights(x.shape[0])
        pos = NODE_BLOCKS[i]
        y = self.tag(pos[0], x, wn)
        if len(pos) == 2:
            y = self.tag(pos[1], torch.relu(y), wn)
        if i != len(NODE_BLOCKS) - 1:
            y = self.inorm(y)
        if y.shape == x.shape:
            y = y + x
        return torch.relu(y)

    def edge_layer(self, i, x):
        """Block i of EdgeModel.forward's loop. Block 0 takes the node features and forms
        [x_src | x_tgt | ea] itself; the others take edge features."""
        x = self.t(x)
        sd = self.sd
        if i == 0:
            x = torch.cat([x[self.src], x[self.tgt], self.ea[:, None]], 1)
            y = self.lin(x, sd["edge_model.blocks.0.0.weight"], sd["edge_model.blocks.0.0.bias"])
            y = self.lnorm(y, sd["edge_model.normaliz.0.weight"], sd["edge_model.normaliz.0.bias"])
            return torch.relu(y)
        p = f"edge_model.blocks.{i}."
        if i == N_EDGE_BLOCKS - 1:
            return self.lin(x, sd[p + "0.weight"], sd[p + "0.bias"])
        y = torch.relu(self.lin(x, sd[p + "0.weight"], sd[p + "0.bias"]))
        y = self.lin(y, sd[p + "2.weight"], sd[p + "2.bias"])
        y = self.lnorm(y, sd[f"edge_model.normaliz.{i}.weight"], sd[f"edge_model.normaliz.{i}.bias"])
        if y.shape == x.shape:
            y = y + x
        return torch.relu(y)

    def standardize(self, v):
        v = self.t(v)
        return torch.abs((v - v.flatten().mean()) / v.std())

    def forward(self, x0):
        """-> (node features after the last block, the E x 1 edge values)."""
        x = self.t(x0)
        for i in range(len(NODE_BLOCKS)):
            x = self.node_layer(i, x)
        e = x
        for i in range(N_EDGE_BLOCKS):
            e = self.edge_layer(i, e)
        return x, self.standardize(e)


def scipy_P(n, src, tgt, vals, C):
    """forward()'s assembly (ali_interp.py:258-281), literally."""
    import scipy.sparse as sp
    coo = sp.coo_matrix((np.asarray(vals).ravel(), (np.asarray(src), np.asarray(tgt))),
                        shape=(n, n))
    P = coo.tolil()
    for j in C:
        P[j, j] = 1.
    P = P.tocsc()
    P = P[:, C]
    return P.tocsr()


def seeded_state_dict(module, seed):
    """Well-scaled random parameters for `module` (an mlamg.interp.ResidualBlock), in place:
    every weight matrix normal with variance 1 / fan_in, split over the K + 1 hops of a TAGConv;
    biases and LayerNorm parameters perturbed so that none is a no-op. -> its state_dict."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 2:
                fan = p.shape[1] * ((HOPS + 1) if ".lins." in name else 1)
                p.copy_(torch.randn(p.shape, generator=g) / np.sqrt(fan))
            elif "normaliz" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return module.state_dict()
