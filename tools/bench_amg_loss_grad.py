"""Time amg_loss, its gradient and the SDDMM kernel; write profiles/mv/amg_loss_grad.json.

  python tools/bench_amg_loss_grad.py [--reps 21] [--out profiles/mv/amg_loss_grad.json] [--quick]

Problems: poisson_2d_5pt(256) with 3 x 3 box aggregates (n_c = 7,396) and poisson_2d_5pt(1024)
with 16 x 16 box aggregates (n_c = 4,096), both with the smoothed-aggregation prolongator
P = (I - 2/3 D^-1 A) Agg. The boxes are chosen so that the coarse operator takes the dense coarse
solve, the only one amg_loss and its gradient run with. For k in {8, 32, 50}, the median over
--reps runs of
  forward        mlamg.loss.amg_loss (device operators and test vectors given; wall time of the
                 call: two-level setup, 6 block cycles, read-back of the history)
  forward+grad   mlamg.loss.amg_loss_and_grad, the same way
  sddmm          one mlamg_sddmm launch on P's pattern (beta = 0 and beta = 1), stream events
                 around the launch, each after a 512 MB cache-flushing read, against the byte
                 model 4 (n + 1) + 4 nnz + 8 nnz (+ 8 nnz if beta != 0) + 8 k n_rows + 8 k n_cols
                 at 8 TB/s
  torch          the same sampled product as (U[rows] * V[cols]).sum(1), timed the same way
"""
from __future__ import annotations

import argparse
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

KS = (8, 32, 50)
PEAK_BPS = 8e12


def timed_us(op, reps, flush):
    """Median time (us) of op() over reps launches, each after a cache flush."""
    s = torch.cuda.current_stream()
    op()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(reps)]
    sink = torch.empty((), dtype=flush.dtype, device=flush.device)
    for e0, e1 in ev:
        torch.sum(flush, dim=0, out=sink)
        e0.record(s)
        op()
        e1.record(s)
    ev[-1][1].synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3


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


def sddmm_model_bytes(P, k, beta):
    n_rows, n_cols = P.shape
    return (4.0 * (n_rows + 1) + 4.0 * P.nnz + 8.0 * P.nnz + (8.0 * P.nnz if beta != 0 else 0.0)
            + 8.0 * k * n_rows + 8.0 * k * n_cols)


def bench_problem(m, box, reps, flush):
    from mlamg import loss, problems
    from mlamg.sparse import DeviceCSR
    A = problems.poisson_2d_5pt(m).tocsr()
    n = A.shape[0]
    agg = sp.csr_matrix(problems.box_aggregates_2d(m, m, box))
    Dinv = sp.diags([1.0 / A.diagonal()], [0])
    P = sp.csr_matrix((sp.eye(n) - (2.0 / 3.0) * Dinv @ A) @ agg)
    P.sum_duplicates()
    P.sort_indices()
    Ad, Pd = DeviceCSR.from_scipy(A), DeviceCSR.from_scipy(P)
    rows_t = torch.as_tensor(np.repeat(np.arange(n), np.diff(P.indptr))).cuda()
    cols_t = torch.as_tensor(P.indices.astype(np.int64)).cuda()
    name = f"poisson_2d_5pt({m}), {box}x{box} boxes"
    out = {"problem": name, "n": n, "n_c": P.shape[1], "nnz_A": int(A.nnz), "nnz_P": int(P.nnz),
           "k": []}
    for k in KS:
        X = torch.randn((n, k), dtype=torch.float64, device="cuda")
        X = X / torch.linalg.vector_norm(X, dim=0)
        t_f = wall_ms(lambda: loss.amg_loss(Pd, Ad, X), reps)
        t_fb = wall_ms(lambda: loss.amg_loss_and_grad(Pd, Ad, X), reps)
        U = torch.randn((n, k), dtype=torch.float64, device="cuda")
        V = torch.randn((P.shape[1], k), dtype=torch.float64, device="cuda")
        o = torch.zeros(P.nnz, dtype=torch.float64, device="cuda")
        t_b0 = timed_us(lambda: Pd.sddmm(U, V, out=o), reps, flush)
        t_b1 = timed_us(lambda: Pd.sddmm(U, V, alpha=1.0, beta=1.0, out=o), reps, flush)
        t_t = timed_us(lambda: (U[rows_t] * V[cols_t]).sum(1), reps, flush)
        ref = (U[rows_t] * V[cols_t]).sum(1)
        got = Pd.sddmm(U, V)
        dev = float((got - ref).abs().max() / ref.abs().max())
        mb0, mb1 = sddmm_model_bytes(P, k, 0.0), sddmm_model_bytes(P, k, 1.0)
        row = {"k": k, "forward_ms": round(t_f, 3), "forward_backward_ms": round(t_fb, 3),
               "backward_over_forward": round(t_fb / t_f, 3),
               "sddmm_beta0_us": round(t_b0, 2), "sddmm_beta1_us": round(t_b1, 2),
               "torch_sampled_us": round(t_t, 2), "sddmm_speedup_over_torch": round(t_t / t_b0, 3),
               "model_bytes_beta0": mb0, "model_bytes_beta1": mb1,
               "model_fraction_beta0": round(mb0 / PEAK_BPS / (t_b0 * 1e-6), 4),
               "model_fraction_beta1": round(mb1 / PEAK_BPS / (t_b1 * 1e-6), 4),
               "max_rel_diff_to_torch": dev}
        out["k"].append(row)
        print(f"{name:34s} k={k:2d}  fwd {t_f:8.2f} ms  fwd+grad {t_fb:8.2f} ms   sddmm "
              f"{t_b0:8.1f} / {t_b1:8.1f} us (beta 0 / 1; {row['model_fraction_beta0']:.3f} of "
              f"model)   torch {t_t:8.1f} us  x{t_t / t_b0:5.2f}", flush=True)
        del X, U, V, o, ref, got
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "amg_loss_grad.json"))
    ap.add_argument("--quick", action="store_true", help="small grids (a functional check)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    flush = torch.ones((512 << 20) // 8, dtype=torch.float64, device="cuda")
    probs = ((48, 3), (64, 4)) if a.quick else ((256, 3), (1024, 16))
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "peak_bytes_per_s": PEAK_BPS,
           "timing": "forward / forward_backward: median wall time of the call, device idle "
                     "before and after; sddmm / torch: median of reps launches between stream "
                     "events, each after a 512 MB cache-flushing read",
           "tot_num_loop": 5, "smoothing": [1, 1], "problems": []}
    for m, box in probs:
        res["problems"].append(bench_problem(m, box, a.reps, flush))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
