"""The fitness the reference's genetic algorithm trains FullAggNet on (utils/train_dataset.py:
81-138), in two batched steps instead of a loop over the grids: FullAggNet.forward_stack on a
GraphBatch (every grid's aggregates and P in a fixed number of launches), then amg_2_v_batch
(every grid's two-level solve in one launch). evaluate_population does the same for a whole
population of weight vectors at once (FullAggNet.forward_population on the stack of members x
grids), with the numbers of the loop over the individuals. The GA itself (selection, mutation,
the worker pool) stays with the caller.
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


def evaluate_population(model, population, batch, alpha=0.3, pre_smoothing_steps=1,
                        post_smoothing_steps=1, aggregation="pyamg", members_per_pass=None):
    """evaluate_dataset for every row of `population` (flat weight vectors in state_dict order)
    at once, as a (P, nb) float array: row p is exactly evaluate_dataset(model, batch, ...,
    weights=population[p]). One FullAggNet.forward_population over the stack of P x nb graphs
    (members_per_pass: its split into passes, which the result does not depend on), one download
    and split of the stacked P, one amg_2_v_batch over all live (member, grid) problems; every
    member's problem on grid g shares the host A, b and start vector of that grid. Where the
    fused solver refuses that joint batch (some member's P has a row of P or P^T beyond its
    slots) the solves are cut into one amg_2_v_batch per member, the loop's own batches, which
    keeps every row exact; only the forward pass is shared then. The model's own weights are
    neither loaded nor changed (evaluate_dataset leaves population[p] loaded)."""
    from types import SimpleNamespace

    from .multigrid import amg_2_v_batch
    model.eval()
    st = model.forward_population(batch, population, alpha, aggregation,
                                  members_per_pass=members_per_pass)
    members, nb = st["failed"].shape
    Ps = _split_P(SimpleNamespace(seg=st["seg"], nb=members * nb),
                  dict(st, failed=st["failed"].reshape(-1)))
    conv = np.ones(members * nb, dtype=np.float64)
    starts = {}
    live, problems = [], []
    for i, P in enumerate(Ps):
        if P is None:
            continue
        g = i % nb
        if g not in starts:
            n = batch.As[g].shape[1]
            x = np.random.RandomState(0).randn(n)
            x /= np.linalg.norm(x, 2)
            starts[g] = (np.zeros(n), x)
        live.append(i)
        problems.append((batch.As[g], P) + starts[g])
    kw = dict(error_tol=1e-6, pre_smoothing_steps=pre_smoothing_steps,
              post_smoothing_steps=post_smoothing_steps)
    res = amg_2_v_batch(problems, fallback=False, **kw) if problems else []
    if res is None:
        # The fused solver plans a batch as a whole: one problem outside its slots sends every
        # problem of the batch to the per-problem engine, whose numbers differ in the last bits.
        # The loop's batches are one member's problems each, so cut there: a member the fused
        # solver takes gets its launch, the others go the way they go in the loop.
        res = []
        for p in range(members):
            own = [q for i, q in zip(live, problems) if i // nb == p]
            res += amg_2_v_batch(own, **kw) if own else []
    for i, r in zip(live, res):
        conv[i] = r[1]
    conv[np.isnan(conv)] = 1.0
    return conv.reshape(members, nb)


def population_fitness_stacked(model, population, batch, alpha=0.3, pre_smoothing_steps=1,
                               post_smoothing_steps=1, aggregation="pyamg",
                               members_per_pass=None):
    """population_fitness from one evaluate_population: 1 / mean(conv factors over the batch)
    per member, the same numbers."""
    conv = evaluate_population(model, population, batch, alpha, pre_smoothing_steps,
                               post_smoothing_steps, aggregation, members_per_pass)
    return np.array([1.0 / np.average(row) for row in conv])
