"""TEST INFRASTRUCTURE ONLY — float64 numpy references of the C-ABI entry points of csrc/gnn.hip
(include/mlamg.h, mlamg_gnn_*), one plain function each, written from the header comments and the
torch_geometric 2.x semantics quoted in oracle/gnn_ref.py. Inputs are the flat arrays the C call
takes; everything is computed in float64. Aggregations run over the edge list itself
(src[e] -> tgt[e], np.add.at): nothing here goes through tptr/teid, so the references do not share
the device path's transposition.
"""
from __future__ import annotations

import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _post(y, act, R):
    """act 0 none, 1 relu; then + R ([rows, 1] broadcasts over the columns)."""
    if act == 1:
        y = np.maximum(y, 0.0)
    if R is not None and y.shape[0]:
        y = y + _f64(R).reshape(y.shape[0], -1)
    return y


def linear(X, W, b=None, act=0, beta=0.0, R=None, Y0=None):
    """Y = act(beta * Y0 + X W^T (+ b)) (+ R); W [N, K]; Y0 is read only when beta != 0."""
    X, W = _f64(X), _f64(W)
    acc = X.reshape(-1, W.shape[1]) @ W.T
    if b is not None:
        acc = acc + _f64(b)
    if beta != 0.0:
        acc = float(beta) * _f64(Y0).reshape(acc.shape) + acc
    return _post(acc, act, R)


def gcn_norm(src, tgt, w, n):
    """gcn_norm without self loops: deg_j = sum of w over the edges with target j, dis = deg^-1/2
    (inf -> 0), wn_e = dis[src_e] w_e dis[tgt_e]. Returns (dis, wn)."""
    w = _f64(w).reshape(-1)
    deg = np.zeros(n)
    np.add.at(deg, np.asarray(tgt, dtype=np.int64), w)
    with np.errstate(divide="ignore"):
        dis = deg ** -0.5
    dis[np.isinf(dis)] = 0.0
    return dis, dis[np.asarray(src, dtype=np.int64)] * w * dis[np.asarray(tgt, dtype=np.int64)]


def propagate(src, tgt, w, X, n):
    """Y[j] = sum over the edges e with tgt_e = j of w_e X[src_e]."""
    X = _f64(X)
    Y = np.zeros((n, X.shape[1]))
    np.add.at(Y, np.asarray(tgt, dtype=np.int64),
              _f64(w).reshape(-1, 1) * X[np.asarray(src, dtype=np.int64)])
    return Y


def instance_norm(X, eps=1e-5):
    """Per channel over the nodes: (x - mean) / sqrt(biased variance + eps)."""
    X = _f64(X)
    mean = X.mean(axis=0, keepdims=True)
    var = ((X - mean) ** 2).mean(axis=0, keepdims=True)
    return (X - mean) / np.sqrt(var + float(eps))


_CHUNK = 1 << 16  # edges per pass: keeps the [E, 16] and [E, Fin, Fout] intermediates small


def nnconv(src, tgt, ea, L1, c1, L2, c2, L3, c3, X, n, Fin, Fout, root, bias, act=0, R=None):
    """NNConv, aggr 'add': W_e = relu(L3 relu(L2 relu(L1 ea_e + c1) + c2) + c3).view(Fin, Fout),
    msg_e = x_src(e) @ W_e, Y = act(sum of the incoming msg + root + bias) (+ R)."""
    src, tgt = np.asarray(src, dtype=np.int64), np.asarray(tgt, dtype=np.int64)
    E = len(src)
    X = _f64(X).reshape(n, Fin)
    out = np.zeros((n, Fout))
    for lo in range(0, E, _CHUNK):
        s, t = src[lo:lo + _CHUNK], tgt[lo:lo + _CHUNK]
        h = np.maximum(_f64(np.asarray(ea).reshape(E, -1)[lo:lo + _CHUNK]) @ _f64(L1).T
                       + _f64(c1), 0.0)
        h = np.maximum(h @ _f64(L2).T + _f64(c2), 0.0)
        We = np.maximum(h @ _f64(L3).T + _f64(c3), 0.0).reshape(len(s), Fin, Fout)
        np.add.at(out, t, np.einsum("ei,eio->eo", X[s], We))
    return _post(out + _f64(root).reshape(n, Fout) + _f64(bias), act, R)


def edge_mlp(src, tgt, X, ea, W1, b1, g, beta, W2, b2, act=0, R=None, eps=1e-5):
    """smallEdgeModel: h = relu(W1 [x_src | x_tgt | ea] + b1), LayerNorm (biased variance, eps
    inside the root) * g + beta, y = W2 h + b2, out = act(y) (+ R)."""
    src, tgt = np.asarray(src, dtype=np.int64), np.asarray(tgt, dtype=np.int64)
    E = len(src)
    X, W1 = _f64(X), _f64(W1)
    H = W1.shape[0]
    W2 = _f64(W2).reshape(-1, H)
    y = np.zeros((E, W2.shape[0]))
    for lo in range(0, E, _CHUNK):
        s, t = src[lo:lo + _CHUNK], tgt[lo:lo + _CHUNK]
        z = np.concatenate([X[s], X[t], _f64(np.asarray(ea).reshape(E, -1)[lo:lo + _CHUNK])],
                           axis=1)
        h = np.maximum(z @ W1.T + _f64(b1), 0.0)
        mean = h.mean(axis=1, keepdims=True)
        var = ((h - mean) ** 2).mean(axis=1, keepdims=True)
        hn = (h - mean) / np.sqrt(var + eps) * _f64(g) + _f64(beta)
        y[lo:lo + _CHUNK] = hn @ W2.T + _f64(b2)
    return _post(y, act, R)


def topk(scores, k):
    """vec[n] = 1 at the k largest scores, idx[k] = those nodes in descending score order, ties to
    the smaller index: a stable descending sort under IEEE comparison (-0.0 == +0.0; the negation
    below maps both zeros to zeros that compare equal, and a stable ascending sort of -s is a
    stable descending sort of s). NaN scores are outside the contract."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    idx = np.argsort(-s, kind="stable")[:k].astype(np.int32)
    vec = np.zeros(len(s), dtype=np.float32)
    vec[idx] = 1.0
    return vec, idx
