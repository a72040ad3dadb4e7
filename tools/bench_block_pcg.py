"""Time the block PCG coarse solve and what it unlocks; write profiles/mv/block_pcg.json.

  python tools/bench_block_pcg.py [--reps 21] [--out profiles/mv/block_pcg.json] [--quick]

Problem: poisson_2d_5pt(1024) with 3 x 3 box aggregates and the smoothed-aggregation prolongator
P = (I - 2/3 D^-1 A) Agg: n_c = 116,964, far beyond the dense coarse solve, so
Hierarchy.two_level gives the coarse operator A_c = P^T A P a PCG solver with an inner SA
hierarchy (csrc/pcg.hip).

  (a) solve      one mlamg_pcg_solve_mv on k random right-hand sides, k in {1, 8, 32, 50},
                 against k successive mlamg_pcg_solve calls on the same solver and the same
                 right-hand sides, in the same run: median of --reps, stream events around the
                 call(s) (the host polls the solver's flag inside, so the interval is the time
                 from the first launch to the end of the last one). The columns are also compared
                 bit for bit.
  (b) loss       mlamg.loss.amg_loss and amg_loss_and_grad on that problem at k in {8, 32, 50}:
                 median wall time of the call (two-level setup with the inner hierarchy, 6 block
                 cycles, the adjoint sweep, read-back), device idle before and after. These
                 calls raised before the block PCG existed, so there is no earlier time; the
                 16 x 16-box figures of profiles/mv/amg_loss_grad.json (n_c = 4,096, dense coarse
                 solve) are copied beside them for scale.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-amg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

KS_SOLVE = (1, 8, 32, 50)
KS_LOSS = (8, 32, 50)


def event_ms(op, reps):
    """Median time (ms) of op() over reps runs between stream events (after one warm-up)."""
    s = torch.cuda.current_stream()
    op()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        op()
        e1.record(s)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def wall_ms(fn, reps):
    """Median wall time (ms) of fn() over reps calls (after one warm-up), device idle before and
    after each."""
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def sa_problem(m, box):
    from mlamg import problems
    A = problems.poisson_2d_5pt(m).tocsr()
    n = A.shape[0]
    agg = sp.csr_matrix(problems.box_aggregates_2d(m, m, box))
    Dinv = sp.diags([1.0 / A.diagonal()], [0])
    P = sp.csr_matrix((sp.eye(n) - (2.0 / 3.0) * Dinv @ A) @ agg)
    P.sum_duplicates()
    P.sort_indices()
    return A, P


def bench_solve(H, reps):
    from mlamg._lib import call, ptr, stream_ptr
    nc = H.Ac.shape[0]
    rows = []
    for k in KS_SOLVE:
        g = torch.Generator(device="cuda").manual_seed(100 + k)
        B = torch.randn((nc, k), dtype=torch.float64, device="cuda", generator=g)
        X = torch.zeros_like(B)
        cols = [B[:, j].contiguous() for j in range(k)]
        xs = [torch.zeros(nc, dtype=torch.float64, device="cuda") for _ in range(k)]
        s = stream_ptr()

        def block():
            call("mlamg_pcg_solve_mv", H.pcg, ptr(B), k, ptr(X), k, k, s)

        def singles():
            for b, x in zip(cols, xs):
                call("mlamg_pcg_solve", H.pcg, ptr(b), ptr(x), s)

        t_block = event_ms(block, reps)
        it = (ctypes.c_int32 * k)()
        call("mlamg_pcg_iters_mv", H.pcg, it, k, s)
        t_single = event_ms(singles, reps)
        same = all(torch.equal(X[:, j], xs[j]) for j in range(k))
        row = {"k": k, "block_ms": round(t_block, 3), "k_single_solves_ms": round(t_single, 3),
               "speedup": round(t_single / t_block, 3), "iterations": sorted(set(it)),
               "columns_bitwise_equal": bool(same)}
        rows.append(row)
        print(f"solve k={k:2d}  block {t_block:9.3f} ms   {k} single solves {t_single:9.3f} ms   "
              f"x{t_single / t_block:5.2f}   iterations {row['iterations']}  bitwise {same}",
              flush=True)
    return rows


def bench_loss(Ad, Pd, n, reps):
    from mlamg import loss
    rows = []
    for k in KS_LOSS:
        g = torch.Generator(device="cuda").manual_seed(200 + k)
        X = torch.randn((n, k), dtype=torch.float64, device="cuda", generator=g)
        X = X / torch.linalg.vector_norm(X, dim=0)
        t_f = wall_ms(lambda: loss.amg_loss(Pd, Ad, X), reps)
        t_fb = wall_ms(lambda: loss.amg_loss_and_grad(Pd, Ad, X), reps)
        rows.append({"k": k, "forward_ms": round(t_f, 3), "forward_backward_ms": round(t_fb, 3),
                     "backward_over_forward": round(t_fb / t_f, 3)})
        print(f"loss  k={k:2d}  fwd {t_f:9.2f} ms   fwd+grad {t_fb:9.2f} ms", flush=True)
    return rows


def dense_coarse_scale():
    """The 16 x 16-box rows of profiles/mv/amg_loss_grad.json (dense coarse solve), if recorded."""
    path = os.path.join(ROOT, "profiles", "mv", "amg_loss_grad.json")
    try:
        with open(path) as fh:
            rec = json.load(fh)
    except OSError:
        return None
    for p in rec.get("problems", ()):
        if "16x16" in p.get("problem", ""):
            return {"problem": p["problem"], "n_c": p["n_c"], "source": "profiles/mv/amg_loss_grad.json",
                    "k": [{"k": r["k"], "forward_ms": r["forward_ms"],
                           "forward_backward_ms": r["forward_backward_ms"]} for r in p["k"]]}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "block_pcg.json"))
    ap.add_argument("--quick", action="store_true", help="a small grid (a functional check)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from mlamg.hierarchy import Hierarchy
    from mlamg.sparse import DeviceCSR
    m, box = (192, 1) if a.quick else (1024, 3)
    A, P = sa_problem(m, box)
    n = A.shape[0]
    Ad, Pd = DeviceCSR.from_scipy(A), DeviceCSR.from_scipy(P)
    H = Hierarchy.two_level(Ad, Pd, omega=2.0 / 3.0)
    assert H.pcg is not None, "the coarse operator must take the PCG coarse solve"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "problem": f"poisson_2d_5pt({m}), {box}x{box} boxes", "n": n, "n_c": P.shape[1],
           "nnz_A_c": int(H.Ac.nnz), "inner_levels": H.inner.n_levels,
           "timing": "solve: median of reps between stream events around the call(s); loss: "
                     "median wall time of the call, device idle before and after",
           "solve": bench_solve(H, a.reps)}
    st = H.coarse_stats()
    res["solver_stats"] = {"not_converged": st["not_converged"], "breakdowns": st["breakdowns"],
                           "max_rel_residual": st["max_rel_residual"]}
    del H
    res["loss"] = {"tot_num_loop": 5, "smoothing": [1, 1], "k": bench_loss(Ad, Pd, n, a.reps),
                   "dense_coarse_for_scale": dense_coarse_scale()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
