"""TEST INFRASTRUCTURE ONLY — the seeded case lists of the per-kernel GNN tests
(tests/test_gnn_kernels_ref_host.py on the CPU, tests/test_gpu_gnn_kernels.py on the device), the
torch restatement of every kernel at a chosen precision, and the tolerance rule both files share.

A case is a dict: "kernel", "id", the flat input arrays of the C call (float32 / int32 numpy) and
its scalar arguments. ref64(case) evaluates oracle/gnn_kernels_ref.py (numpy, float64);
restate(case, dtype) evaluates the torch restatement (oracle/gnn_ref.py functions, or
torch.nn.functional where gnn_ref wants a module) in float32 or float64. The float32 run's distance
from ref64 is err_ref32, the error of a correct fp32 evaluation: the yardstick of the device tests.

Tolerance rule, per floating-point output tensor: scale = max|ref64|, and
    err_dev = max|dev - ref64| <= max(4 err_ref32, 4 * 2^-24 * scale).
The second term is the floor where the fp32 restatement happens to be exact (a few roundings of
the result); the factor 4 is a margin for the different summation orders (fma chains in edge order
on the device, blocked sums in torch), the same for every case.

Conditioning caps (asserted on the CPU by the host test, so that whether a case list is admissible
is not decided by the kernel under test):
  * instance_norm: every non-constant channel has |mean| <= 10 std — the subtraction x - mean then
    loses at most ~3.5 bits, fp32 stays well conditioned. Exactly constant channels (and n = 1)
    are compared apart, against 0 with scale |c| / sqrt(eps).
  * edge_mlp, H >= 2: per edge |mean_h| <= 10 sqrt(var_h + eps), the same argument for LayerNorm
    (H = 1 has h - mean == 0 exactly in any precision).
"""
from __future__ import annotations

import functools
import itertools
import types

import numpy as np

from . import gnn_kernels_ref as kref

F32_EPS = 2.0 ** -24  # unit roundoff of float32
T_CAP = 4 * (1 << 20) + 5  # first item count past 4 items x 2^20 blocks, and odd


# ------------------------------------------------------------------------------------- graphs
def make_graph(n, src, tgt, w):
    """Edges in row-major (src, tgt) order like the stored entries of a CSR matrix, plus the
    device path's index of each target's incoming edges (ascending source): tptr / teid."""
    src, tgt = np.asarray(src, dtype=np.int32), np.asarray(tgt, dtype=np.int32)
    assert np.all(np.lexsort((tgt, src)) == np.arange(len(src))), "edges must be row-major"
    tptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(tgt, minlength=n), out=tptr[1:])
    teid = np.argsort(tgt, kind="stable").astype(np.int32)
    return types.SimpleNamespace(n=n, E=len(src), src=src, tgt=tgt, tptr=tptr, teid=teid,
                                 w=np.asarray(w, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def dir7():
    """7 nodes, directed, non-symmetric pattern and weights: node 0 has no incoming edge, node 6
    no outgoing edge, node 3's only incoming edge is its self-loop, (1,2) and (4,5) carry the
    same weight, (1,2) / (2,1) are both present with different weights."""
    e = [(0, 1, 0.5), (0, 2, 1.5), (0, 4, 0.7),
         (1, 1, 1.0), (1, 2, 0.3), (1, 5, 2.0),
         (2, 1, 0.9), (2, 4, 1.1), (2, 6, 0.6),
         (3, 3, 1.3), (3, 4, 0.8), (3, 5, 0.4),
         (4, 2, 1.7), (4, 5, 0.3), (4, 6, 1.2),
         (5, 1, 0.2), (5, 4, 1.9), (5, 6, 0.45)]
    s, t, w = zip(*e)
    return make_graph(7, s, t, w)


@functools.lru_cache(maxsize=None)
def ragged301():
    """301 nodes, random directed pattern, in-degrees 0..40 (both ends present), self-loops at
    every third node that has edges, weights in [0.1, 2]."""
    n = 301
    rs = np.random.RandomState(301)
    indeg = rs.randint(0, 41, n)
    indeg[5], indeg[17] = 0, 40
    src, tgt = [], []
    for j in range(n):
        s = rs.choice(n, indeg[j], replace=False)
        if j % 3 == 0 and indeg[j] > 0 and j not in s:
            s[0] = j
        src.append(s)
        tgt.append(np.full(indeg[j], j))
    src, tgt = np.concatenate(src), np.concatenate(tgt)
    order = np.lexsort((tgt, src))
    return make_graph(n, src[order], tgt[order], rs.uniform(0.1, 2.0, len(src)))


@functools.lru_cache(maxsize=None)
def empty5():
    return make_graph(5, [], [], [])


def ring(T):
    """Directed ring e: e -> e + 1 (mod T): one incoming edge per node, weight varying with the
    index. tptr / teid in closed form (node j's incoming edge is j - 1); src = 0..T-1 is a view
    of tptr = 0..T."""
    tptr = np.arange(T + 1, dtype=np.int32)
    a = tptr[:T]
    tgt = a + 1
    tgt[-1] = 0
    w = (0.1 + 1.9 * ((a.astype(np.float64) * 0.6180339887498949) % 1.0)).astype(np.float32)
    teid = a - 1
    teid[0] = T - 1
    return types.SimpleNamespace(n=T, E=T, src=a, tgt=tgt, tptr=tptr, teid=teid, w=w)


GRAPHS = {"dir7": dir7, "ragged301": ragged301, "empty5": empty5}


def swapped(g):
    """The same edges with every direction reversed (what a kernel that mixed up src and tgt
    would compute on), kept in the original edge order: only for the references."""
    return types.SimpleNamespace(n=g.n, E=g.E, src=g.tgt, tgt=g.src, w=g.w)


# -------------------------------------------------------------------------------------- cases
def _seed(*key):
    """A seed from the case's integers (hash() of str is salted per process: ints only)."""
    s = 12345
    for k in key:
        s = (s * 1000003 + int(k) + 7) % (2 ** 31 - 1)
    return np.random.RandomState(s)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _res(rs, rows, cols, kind):
    """residual none / rc1 / full."""
    if kind == "none":
        return None
    return _f(rs.randn(rows, 1 if kind == "rc1" else cols))


LINEAR_SHAPES = ((1, 1, 1), (5, 7, 3), (301, 64, 33), (130, 160, 64), (67, 1, 64), (0, 4, 4))
# (bias, act, beta, residual): every value of every option appears at every shape
LINEAR_COMBOS = ((1, 0, 0.0, "none"), (0, 1, 1.0, "rc1"), (1, 1, 1.0, "full"),
                 (0, 0, 0.0, "full"))


@functools.lru_cache(maxsize=None)
def linear_cases():
    out = []
    for si, (M, K, N) in enumerate(LINEAR_SHAPES):
        for ci, (bias, act, beta, res) in enumerate(LINEAR_COMBOS):
            rs = _seed(1, si, ci)
            out.append(dict(
                kernel="linear", id=f"M{M}-K{K}-N{N}-b{bias}-act{act}-beta{int(beta)}-{res}",
                M=M, K=K, N=N, X=_f(rs.randn(M, K)), W=_f(rs.randn(N, K) / np.sqrt(K)),
                b=_f(rs.uniform(-0.5, 0.5, N)) if bias else None, act=act, beta=beta,
                R=_res(rs, M, N, res), Y0=_f(rs.randn(M, N)) if beta else None))
    return out


GRAPH_F = (1, 3, 64)


@functools.lru_cache(maxsize=None)
def gcn_norm_cases():
    return [dict(kernel="gcn_norm", id=name, graph=g()) for name, g in GRAPHS.items()]


@functools.lru_cache(maxsize=None)
def propagate_cases():
    out = []
    for gi, (name, g) in enumerate(GRAPHS.items()):
        for F in GRAPH_F:
            out.append(dict(kernel="propagate", id=f"{name}-F{F}", graph=g(), F=F,
                            w=g().w, X=_f(_seed(2, gi, F).randn(g().n, F))))
    return out


INORM_N = (1, 2, 255, 256, 257, 1000)
INORM_F = (1, 3, 64, 130)


@functools.lru_cache(maxsize=None)
def instance_norm_cases():
    """Random channels std_f (u_f + z) with z standardised over the nodes and |u_f| <= 9.5: the
    mean sits up to 9.5 standard deviations off zero. For F >= 3 the last channel is the exact
    constant 1/n (the reference graphs' own node input); with n = 1 every channel is constant."""
    out = []
    for n, F in itertools.product(INORM_N, INORM_F):
        rs = _seed(3, n, F)
        z = rs.randn(n, F)
        if n >= 2:
            z = (z - z.mean(axis=0)) / z.std(axis=0)
        else:
            z[:] = 0.0
        X = _f(rs.uniform(0.5, 2.0, F) * (rs.uniform(-9.5, 9.5, F) + z))
        const = np.zeros(F, dtype=bool)
        if n == 1:
            const[:] = True
        elif F >= 3:
            X[:, F - 1] = np.float32(1.0 / n)
            const[F - 1] = True
        out.append(dict(kernel="instance_norm", id=f"n{n}-F{F}", n=n, F=F, X=X, eps=1e-5,
                        const=const))
    return out


NNCONV_SHAPES = ((1, 1, 1), (1, 64, 1), (3, 15, 2), (64, 16, 2), (5, 17, 3), (64, 64, 2),
                 (64, 1, 2))
ACT_RES = ((1, "none"), (0, "rc1"), (1, "full"), (0, "none"), (1, "rc1"), (0, "full"))


def _nnconv_case(gname, g, Fin, Fout, fe, act, res, key):
    rs = _seed(4, *key)
    X = _f(rs.randn(g.n, Fin))
    Wroot = _f(rs.randn(Fout, Fin) / np.sqrt(Fin))
    return dict(
        kernel="nnconv", id=f"{gname}-Fin{Fin}-Fout{Fout}-fe{fe}-act{act}-{res}", graph=g,
        Fin=Fin, Fout=Fout, fe=fe, ea=_f(rs.uniform(0.1, 2.0, (g.E, fe))),
        L1=_f(0.7 * rs.randn(4, fe)), c1=_f(rs.uniform(0.05, 0.3, 4)),
        L2=_f(0.5 * rs.randn(16, 4)), c2=_f(rs.uniform(0.05, 0.3, 16)),
        L3=_f(0.25 * rs.randn(Fin * Fout, 16)), c3=_f(rs.uniform(0.05, 0.3, Fin * Fout)),
        X=X, root=_f(X @ Wroot.T), bias=_f(rs.uniform(-0.3, 0.3, Fout)), act=act,
        R=_res(rs, g.n, Fout, res))


@functools.lru_cache(maxsize=None)
def nnconv_cases():
    out = []
    for si, (Fin, Fout, fe) in enumerate(NNCONV_SHAPES):
        act, res = ACT_RES[si % len(ACT_RES)]
        out.append(_nnconv_case("ragged301", ragged301(), Fin, Fout, fe, act, res, (0, si)))
    for si, (Fin, Fout, fe) in enumerate(NNCONV_SHAPES[:3]):
        act, res = ACT_RES[(si + 3) % len(ACT_RES)]
        out.append(_nnconv_case("dir7", dir7(), Fin, Fout, fe, act, res, (1, si)))
    for si, (act, res) in enumerate(((1, "full"), (0, "none"))):
        out.append(_nnconv_case("empty5", empty5(), 3, 15, 2, act, res, (2, si)))
    return out


EDGE_MLP_SHAPES = ((1, 1, 1, 1), (1, 2, 5, 2), (64, 2, 64, 2), (7, 3, 63, 4), (2, 1, 64, 3),
                   (79, 2, 64, 1))


def _edge_mlp_case(gname, g, F, fe, H, C, act, res, key):
    rs = _seed(5, *key)
    K = 2 * F + fe
    return dict(
        kernel="edge_mlp", id=f"{gname}-F{F}-fe{fe}-H{H}-C{C}-act{act}-{res}", graph=g, F=F,
        fe=fe, H=H, C=C, X=_f(rs.randn(g.n, F)), ea=_f(rs.uniform(0.1, 2.0, (g.E, fe))),
        W1=_f(rs.randn(H, K) / np.sqrt(K)), b1=_f(rs.uniform(0.05, 0.3, H)),
        g=_f(rs.uniform(0.5, 1.5, H)), beta=_f(rs.uniform(-0.5, 0.5, H)),
        W2=_f(rs.randn(C, H) / np.sqrt(H)), b2=_f(rs.uniform(-0.3, 0.3, C)), act=act,
        R=_res(rs, g.E, C, res))


@functools.lru_cache(maxsize=None)
def edge_mlp_cases():
    out = []
    for gi, (gname, g) in enumerate((("ragged301", ragged301()), ("dir7", dir7()))):
        for si, (F, fe, H, C) in enumerate(EDGE_MLP_SHAPES):
            act, res = ACT_RES[(si + 2 * gi) % len(ACT_RES)]
            out.append(_edge_mlp_case(gname, g, F, fe, H, C, act, res, (gi, si)))
    return out


TOPK_N = (1, 6, 257, 5000)
TOPK_KINDS = ("random", "equal", "ties", "relu70", "signed_zero", "inf")


def topk_scores(kind, n):
    """None where the kind does not exist at that n."""
    rs = _seed(6, TOPK_KINDS.index(kind), n)
    if kind == "random":
        s = rs.randn(n)
    elif kind == "equal":
        s = np.full(n, 0.75)
    elif kind == "ties":  # the explicit-ties vector of tests/test_gpu_gnn.py
        s = np.array([1.0, 3.0, 3.0, 0.0, 3.0, -1.0]) if n == 6 else None
    elif kind == "relu70":
        s = np.where(rs.uniform(size=n) < 0.7, 0.0, rs.uniform(0.0, 1.0, n))
    elif kind == "signed_zero":  # zeros of both signs among a few positive and negative scores
        s = rs.choice([0.0, -0.0, 0.0, -0.0, 0.5, -0.5], n)
        if n >= 2:
            s[0], s[1] = -0.0, 0.0
    else:
        s = rs.randn(n)
        s[rs.randint(0, n, max(1, n // 8))] = np.inf
        s[rs.randint(0, n, max(1, n // 8))] = -np.inf
    return None if s is None else _f(s)


@functools.lru_cache(maxsize=None)
def topk_cases():
    out = [dict(kernel="topk", id="signed_zero-pair-k1", kind="signed_zero",
                scores=_f([-0.0, 0.0]), k=1)]
    for kind, n in itertools.product(TOPK_KINDS, TOPK_N):
        s = topk_scores(kind, n)
        if s is None:
            continue
        for k in sorted({0, 1, n // 10, n}):
            out.append(dict(kernel="topk", id=f"{kind}-n{n}-k{k}", kind=kind, scores=s, k=k))
    return out


def gridcap_case(kernel, T=T_CAP):
    """The narrowest case of a wave-per-item kernel at T items (default: the first count a grid
    capped at 2^20 blocks of 4 waves would not cover). propagate and nnconv run on the directed
    ring of T nodes; edge_mlp on T edges over 1,000 nodes with H = 2, its two hidden units kept
    apart by construction (h0 in [1, 3.5], h1 in [0.2, 0.6]) so that LayerNorm is well
    conditioned on every edge. Arrays that may coincide do (the ring's src is a view of tptr;
    nnconv: root weight 1, so root = X, and R = X; edge_mlp: R = ea), which keeps each case's
    T-long arrays at six or fewer: under 100 MiB on the device."""
    rs = _seed(7, T)
    if kernel == "propagate":
        g = ring(T)
        return dict(kernel="propagate", id=f"ring{T}-F1", graph=g, F=1, w=g.w,
                    X=_f(rs.randn(T, 1)))
    if kernel == "nnconv":
        g = ring(T)
        X = _f(rs.randn(T, 1))
        return dict(kernel="nnconv", id=f"ring{T}-1-1-1", graph=g, Fin=1, Fout=1, fe=1,
                    ea=g.w.reshape(T, 1), L1=_f(0.7 * rs.randn(4, 1)),
                    c1=_f(rs.uniform(0.05, 0.3, 4)), L2=_f(0.5 * rs.randn(16, 4)),
                    c2=_f(rs.uniform(0.05, 0.3, 16)), L3=_f(0.25 * rs.randn(1, 16)),
                    c3=_f(rs.uniform(0.05, 0.3, 1)), X=X, root=X, bias=_f([0.1]), act=1, R=X)
    assert kernel == "edge_mlp"
    n = 1000
    a = np.arange(T, dtype=np.int64)
    g = types.SimpleNamespace(n=n, E=T, src=(a % n).astype(np.int32),
                              tgt=((a * 7 + a // n) % n).astype(np.int32))
    ea = _f(rs.uniform(0.1, 2.0, (T, 1)))
    return dict(kernel="edge_mlp", id=f"edges{T}-1-1-2-1", graph=g, F=1, fe=1, H=2, C=1,
                X=_f(rs.uniform(0.5, 1.5, (n, 1))), ea=ea,
                W1=_f([[1.0, 0.5, 0.5], [0.2, 0.1, 0.05]]), b1=_f([0.2, 0.05]),
                g=_f([1.25, 0.75]), beta=_f([0.3, -0.2]), W2=_f([[0.8, -0.6]]), b2=_f([0.1]),
                act=1, R=ea)


# ---------------------------------------------------------------------------------- evaluation
def ref64(c):
    """name -> float64 numpy reference of every output of the case's kernel."""
    k = c["kernel"]
    if k == "linear":
        return {"Y": kref.linear(c["X"], c["W"], c["b"], c["act"], c["beta"], c["R"], c["Y0"])}
    g = c.get("graph")
    if k == "gcn_norm":
        dis, wn = kref.gcn_norm(g.src, g.tgt, g.w, g.n)
        return {"dis": dis, "wn": wn}
    if k == "propagate":
        return {"Y": kref.propagate(g.src, g.tgt, c["w"], c["X"], g.n)}
    if k == "instance_norm":
        return {"Y": kref.instance_norm(c["X"], c["eps"])}
    if k == "nnconv":
        return {"Y": kref.nnconv(g.src, g.tgt, c["ea"], c["L1"], c["c1"], c["L2"], c["c2"],
                                 c["L3"], c["c3"], c["X"], g.n, c["Fin"], c["Fout"], c["root"],
                                 c["bias"], c["act"], c["R"])}
    if k == "edge_mlp":
        return {"out": kref.edge_mlp(g.src, g.tgt, c["X"], c["ea"], c["W1"], c["b1"], c["g"],
                                     c["beta"], c["W2"], c["b2"], c["act"], c["R"])}
    raise KeyError(k)


_TCHUNK = 1 << 18


def restate(c, dtype):
    """The torch restatement of the case's kernel with inputs and weights cast to dtype
    ("float32" / "float64"); name -> numpy array (in that dtype)."""
    import torch
    import torch.nn.functional as F

    from . import gnn_ref
    dt = getattr(torch, dtype)

    def t(a):
        return None if a is None else torch.as_tensor(np.asarray(a)).to(dt)

    def li(a):
        return torch.as_tensor(np.asarray(a, dtype=np.int64))

    def post(y, rows):
        if c["act"] == 1:
            y = F.relu(y)
        if c["R"] is not None and rows:
            y = y + t(c["R"]).reshape(rows, -1)
        return y

    k = c["kernel"]
    g = c.get("graph")
    with torch.no_grad():
        if k == "linear":
            y = F.linear(t(c["X"]), t(c["W"]), t(c["b"]))
            if c["beta"] != 0.0:
                y = c["beta"] * t(c["Y0"]) + y
            out = {"Y": post(y, c["M"])}
        elif k == "gcn_norm":
            w = t(g.w)
            deg = gnn_ref._scatter_add(w, li(g.tgt), g.n)
            dis = deg.pow(-0.5)
            dis[torch.isinf(dis)] = 0.0
            out = {"dis": dis, "wn": gnn_ref.gcn_norm((li(g.src), li(g.tgt)), w, g.n)}
        elif k == "propagate":
            x = t(c["X"])
            out = {"Y": gnn_ref._scatter_add(t(c["w"]).view(-1, 1) * x[li(g.src)], li(g.tgt),
                                             g.n)}
        elif k == "instance_norm":
            x = t(c["X"])
            if c["n"] > 1:
                y = gnn_ref.instance_norm(x)
            else:  # F.instance_norm refuses a single element; the same formula by hand
                mean = x.mean(dim=0, keepdim=True)
                var = ((x - mean) ** 2).mean(dim=0, keepdim=True)
                y = (x - mean) / torch.sqrt(var + c["eps"])
            out = {"Y": y}
        elif k == "nnconv":  # gnn_ref.nnconv on bare tensors
            x = t(c["X"])
            ea = t(c["ea"]).reshape(g.E, c["fe"])
            agg = torch.zeros((g.n, c["Fout"]), dtype=dt)
            for lo in range(0, g.E, _TCHUNK):
                s, tg = li(g.src[lo:lo + _TCHUNK]), li(g.tgt[lo:lo + _TCHUNK])
                h = F.relu(F.linear(ea[lo:lo + _TCHUNK], t(c["L1"]), t(c["c1"])))
                h = F.relu(F.linear(h, t(c["L2"]), t(c["c2"])))
                h = F.relu(F.linear(h, t(c["L3"]), t(c["c3"])))
                weight = h.view(-1, c["Fin"], c["Fout"])
                agg.index_add_(0, tg, torch.matmul(x[s].unsqueeze(1), weight).squeeze(1))
            out = {"Y": post(agg + t(c["root"]).reshape(g.n, -1) + t(c["bias"]), g.n)}
        elif k == "edge_mlp":  # gnn_ref.edge_model + smallEdgeModel's Sequential
            x = t(c["X"])
            ea = t(c["ea"]).reshape(g.E, c["fe"])
            ys = []
            for lo in range(0, g.E, _TCHUNK):
                s, tg = li(g.src[lo:lo + _TCHUNK]), li(g.tgt[lo:lo + _TCHUNK])
                h = F.relu(F.linear(torch.cat([x[s], x[tg], ea[lo:lo + _TCHUNK]], 1),
                                    t(c["W1"]), t(c["b1"])))
                h = F.layer_norm(h, (c["H"],), t(c["g"]), t(c["beta"]), 1e-5)
                ys.append(F.linear(h, t(c["W2"]), t(c["b2"])))
            y = torch.cat(ys) if ys else torch.zeros((0, c["C"]), dtype=dt)
            out = {"out": post(y, g.E)}
        else:
            raise KeyError(k)
    return {name: v.numpy() for name, v in out.items()}


def restate_topk(scores, k):
    """gnn_ref.topk_vec and the order behind it: (vec float32, idx int32)."""
    import torch

    from . import gnn_ref
    s = torch.as_tensor(np.asarray(scores))
    idx = torch.sort(s, descending=True, stable=True).indices[:k]
    return gnn_ref.topk_vec(s, k).numpy(), idx.numpy().astype(np.int32)


def tolerance(err32, scale):
    return max(4.0 * err32, 4.0 * F32_EPS * scale)


def _amax(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return float(a.max()) if a.size else 0.0


def parts(c, name, arr):
    """The tensors of output `name` that the rule applies to, as (label, array, scale or None):
    instance_norm is split into its random channels (scale = max|ref64|) and its constant ones
    (reference 0; scale = max|c| / sqrt(eps))."""
    arr = np.asarray(arr)
    if c["kernel"] != "instance_norm":
        return [(name, arr, None)]
    const = c["const"]
    out = []
    if (~const).any():
        out.append((name, arr[:, ~const], None))
    if const.any():
        cmax = _amax(c["X"][:, const])
        out.append((name + "[const]", arr[:, const], cmax / np.sqrt(c["eps"])))
    return out


def yardsticks(c):
    """For every tensor of the case: label -> (ref64, err_ref32, scale, tolerance)."""
    r64, r32 = ref64(c), restate(c, "float32")
    out = {}
    for name in r64:
        for (label, ref, scale), (_, got, _) in zip(parts(c, name, r64[name]),
                                                    parts(c, name, r32[name])):
            ref = ref.reshape(got.shape)
            scale = _amax(ref) if scale is None else scale
            err32 = _amax(got.astype(np.float64) - ref)
            out[label] = (ref, err32, scale, tolerance(err32, scale))
    return out


def judge(c, dev, yard=None):
    """Apply the rule to the device outputs {name: array}. Returns a list of
    (label, err_dev, err_ref32, scale, tol, ok); NaN in dev makes err_dev NaN and ok False."""
    yard = yard or yardsticks(c)
    rows = []
    for name, arr in dev.items():
        for label, got, _ in parts(c, name, arr):
            ref, err32, scale, tol = yard[label]
            d = got.astype(np.float64).reshape(ref.shape) - ref
            err = float(np.abs(d).max()) if d.size else 0.0
            rows.append((label, err, err32, scale, tol, bool(err <= tol)))
    return rows
