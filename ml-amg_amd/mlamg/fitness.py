"""The fitness the reference's genetic algorithm trains FullAggNet on (utils/train_dataset.py:
81-138), in two batched steps instead of a loop over the grids: FullAggNet.forward_stack on a
GraphBatch (every grid's aggregates and P in a fixed number of launches), then amg_2_v_batch
(every grid's two-level solve in one launch). The GA itself (selection, mutation, the worker
pool) stays with the caller.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch


def weights_as_dict(model, weights):
    """ns.ga.torch.model_weights_as_dict: a flat vector in state_dict order -> a state_dict with
    the model's shapes and dtypes (model_weights_as_vector is the inverse, weights_as_vector)."""
    weights = np.asarray(weights).reshape(-1)
    sd = model.state_dict()
    total = sum(v.numel() for v in sd.values())
    if weights.size != total:
        raise ValueError(f"weight vector has {weights.size} entries, the model {total}")
    out, at = {}, 0
    for name, v in sd.items():
        w = weights[at:at + v.numel()]
        out[name] = torch.as_tensor(np.ascontiguousarray(w)).reshape(v.shape).to(v.dtype)
        at += v.numel()
    return out


def weights_as_vector(model):
    """ns.ga.torch.model_weights_as_vector: every state_dict tensor, flattened, in order."""
    return np.concatenate([v.detach().cpu().numpy().reshape(-1)
                           for v in model.state_dict().values()])


def _split_P(batch, st):
    """The stacked P of forward_stack as one scipy CSR (fp32 values, local columns) per graph;
    None for a failed graph. One download for the whole batch."""
    P = st["P"].to_scipy()
    P.sort_indices()  # the loop's P comes out of a coalesced COO: columns ascending
    seg, kp = batch.seg.host, st["kptr"].host
    out = []
    for g in range(batch.nb):
        if st["failed"][g]:
            out.append(None)
            continue
        a, b = P.indptr[seg[g]], P.indptr[seg[g + 1]]
        out.append(sp.csr_matrix((P.data[a:b].astype(np.float32), P.indices[a:b] - kp[g],
                                  P.indptr[seg[g]:seg[g + 1] + 1] - a),
                                 shape=(int(seg[g + 1] - seg[g]), int(kp[g + 1] - kp[g]))))
    return out


def evaluate_dataset(model, batch, alpha=0.3, pre_smoothing_steps=1, post_smoothing_steps=1,
                     weights=None, aggregation="pyamg"):
    """train_dataset.py:81-117 on a GraphBatch: the convergence factor of amg_2_v(A, P, b = 0,
    x = RandomState(0).randn(n) / ||.||_2, error_tol=1e-6) with P from the model, per grid, as
    a float array. A grid the model fails on (a node reached by no seed: the reference's
    `except` branch) scores 1.0, and so does a NaN. weights: an optional flat vector in
    state_dict order (model_weights_as_vector's layout), loaded before the run."""
    from .multigrid import amg_2_v_batch
    if weights is not None:
        model.load_state_dict(weights_as_dict(model, weights))
    model.eval()
    st = model.forward_stack(batch, alpha, aggregation)
    Ps = _split_P(batch, st)
    conv = np.ones(batch.nb, dtype=np.float64)
    live, problems = [], []
    for g, (A, P) in enumerate(zip(batch.As, Ps)):
        if P is None:
            continue
        n = A.shape[1]
        x = np.random.RandomState(0).randn(n)
        x /= np.linalg.norm(x, 2)
        live.append(g)
        problems.append((A, P, np.zeros(n), x))
    res = amg_2_v_batch(problems, error_tol=1e-6, pre_smoothing_steps=pre_smoothing_steps,
                        post_smoothing_steps=post_smoothing_steps) if problems else []
    for g, r in zip(live, res):
        conv[g] = r[1]
    conv[np.isnan(conv)] = 1.0
    return conv


def population_fitness(model, population, batch, alpha=0.3, pre_smoothing_steps=1,
                       post_smoothing_steps=1, aggregation="pyamg"):
    """fitness() of train_dataset.py:120-138 with loss_relative_measure=False for every row of
    `population` (one flat weight vector each): 1 / mean(conv factors over the batch)."""
    return np.array([1.0 / np.average(evaluate_dataset(
        model, batch, alpha, pre_smoothing_steps, post_smoothing_steps, weights=w,
        aggregation=aggregation)) for w in population])
