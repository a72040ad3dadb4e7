"""Time the Chebyshev polynomial smoother against what it replaces; write
profiles/smoothers/chebyshev.json.

  python tools/bench_chebyshev.py [--reps 21] [--out profiles/smoothers/chebyshev.json] [--quick]

On poisson_2d_5pt(1024) and poisson_3d_7pt(128) (--quick: 256^2 and 32^3), in one run:
  (a) one degree-3 sweep (mlamg_poly_sweep: 3 passes over A) against three mlamg_jacobi sweeps on
      the same operator handle, and the sweep's three launches one by one;
  (b) the pyamg_sa V(1,1) cycle with Chebyshev degree 3 against the recipe's symmetric block
      Gauss-Seidel cycle (code this smoother does not touch), with each cycle's residual
      reduction (geometric mean over cycles 4..10 from a random right-hand side);
  (c) gmres to 1e-8 on both hierarchies: Krylov steps and wall time, and gmres_multi at k = 8;
  (d) the block cycle at k = 8 against eight single cycles (Chebyshev hierarchy).
Timing: a warm-up, then medians over `reps` repetitions, stream events around the launches; the
Krylov solves are wall time around a synchronised call. Nothing is gated on a ratio."""
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
import torch  # noqa: E402


def timed_us(op, reps):
    """Median time (us) of op() over reps repetitions."""
    s = torch.cuda.current_stream()
    op()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(s)
        op()
        e1.record(s)
    ev[-1][1].synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3


def wall_ms(op):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = op()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def reduction(hist):
    h = np.asarray(hist)
    if len(h) < 5:
        return None
    r = h[4:] / h[3:-1]
    return float(np.exp(np.mean(np.log(r))))


def bench_grid(name, A, reps):
    from mlamg import hierarchy, multigrid
    from mlamg._lib import call, ptr, stream_ptr
    out = {"grid": name, "n": int(A.shape[0]), "nnz": int(A.nnz)}
    n = A.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(7)
    b = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    t0 = time.perf_counter()
    Hg = hierarchy.Hierarchy.pyamg_sa(A)
    torch.cuda.synchronize()
    out["setup_gauss_seidel_s"] = round(time.perf_counter() - t0, 3)
    print(f"[{name}] gauss-seidel hierarchy: {out['setup_gauss_seidel_s']} s", flush=True)
    np.random.seed(0)
    t0 = time.perf_counter()
    Hc = hierarchy.Hierarchy.pyamg_sa(A, smoother=("chebyshev", {"degree": 3}),
                                      smoother_rho="arnoldi")
    torch.cuda.synchronize()
    out["setup_chebyshev_s"] = round(time.perf_counter() - t0, 3)
    out["levels"] = [r for r in Hc.describe()]
    out["rho_A"] = [L.rho_A for L in Hc.levels]
    print(f"[{name}] chebyshev hierarchy: {out['setup_chebyshev_s']} s, "
          f"{Hc.n_levels} levels", flush=True)

    # (a) one sweep against three Jacobi sweeps, same handle
    L0 = Hc.levels[0]
    S = L0.poly
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    tmp = torch.empty_like(x)
    dinv = L0.A.diag_inv(2.0 / 3.0)
    a = {"format": L0.A.get_format()[0]}
    a["chebyshev_sweep_us"] = timed_us(lambda: S.sweep(x, b, 1), reps)
    a["jacobi_3_sweeps_us"] = timed_us(
        lambda: call("mlamg_jacobi", L0.A.handle, ptr(dinv), ptr(b), ptr(x), ptr(tmp), 3,
                     stream_ptr()), reps)
    a["jacobi_2_sweeps_us"] = timed_us(
        lambda: call("mlamg_jacobi", L0.A.handle, ptr(dinv), ptr(b), ptr(x), ptr(tmp), 2,
                     stream_ptr()), reps)
    a["residual_us"] = timed_us(
        lambda: call("mlamg_residual", L0.A.handle, ptr(b), ptr(x), ptr(tmp), None,
                     stream_ptr()), reps)
    a["chebyshev_sweep_from_zero_us"] = timed_us(lambda: S.sweep(x, b, 1, x_is_zero=True), reps)
    a["ratio_chebyshev_over_jacobi3"] = a["chebyshev_sweep_us"] / a["jacobi_3_sweeps_us"]
    out["sweep"] = a
    print(f"[{name}] sweep {a}", flush=True)

    # (b) cycles
    cyc = {}
    for tag, H in (("gauss_seidel", Hg), ("chebyshev", Hc)):
        xz = torch.zeros_like(b)
        hist = H.cycle(b, xz, 10)
        xs = torch.zeros_like(b)
        us = timed_us(lambda: H.cycle_async(b, xs, 1, zero_rhs=False), reps)
        cyc[tag] = {"cycle_ms": us / 1e3, "residual_reduction_per_cycle": reduction(hist),
                    "history": [float(v) for v in hist]}
        print(f"[{name}] cycle {tag}: {us / 1e3:.3f} ms, reduction "
              f"{cyc[tag]['residual_reduction_per_cycle']}", flush=True)
    out["cycle"] = cyc

    # (c) GMRES to 1e-8
    Hg.enable_block_gauss_seidel()
    B8 = torch.randn((n, 8), dtype=torch.float64, device="cuda", generator=gen)
    gm = {}
    for tag, H in (("gauss_seidel", Hg), ("chebyshev", Hc)):
        H.gmres(b, rtol=1e-8, restart=30)  # warm-up (workspace, graphs)
        ms, (xsol, info) = wall_ms(lambda: H.gmres(b, rtol=1e-8, restart=30, return_info=True))
        H.gmres_multi(B8, rtol=1e-8, restart=30)
        ms8, (_, info8) = wall_ms(lambda: H.gmres_multi(B8, rtol=1e-8, restart=30,
                                                        return_info=True))
        gm[tag] = {"steps": int(info["inner_iters"]), "info": int(info["info"]), "wall_ms": ms,
                   "multi_k8_steps": [int(v) for v in info8["inner_iters"]],
                   "multi_k8_wall_ms": ms8}
        print(f"[{name}] gmres {tag}: {gm[tag]}", flush=True)
    out["gmres"] = gm

    # (d) block cycle at k = 8 against eight single cycles
    X8 = torch.zeros_like(B8)
    cols = [B8[:, j].contiguous() for j in range(8)]
    xs8 = [torch.zeros_like(b) for _ in range(8)]

    def singles():
        for j in range(8):
            Hc.cycle_async(cols[j], xs8[j], 1, zero_rhs=False)

    blk = {"block_k8_ms": timed_us(lambda: Hc.cycle_multi(B8, X8, 1, history=False), reps) / 1e3,
           "eight_single_ms": timed_us(singles, reps) / 1e3}
    blk["speedup"] = blk["eight_single_ms"] / blk["block_k8_ms"]
    out["block_cycle"] = blk
    print(f"[{name}] block cycle {blk}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smoothers", "chebyshev.json"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    from mlamg import problems
    grids = ((("poisson_2d_5pt(256)", problems.poisson_2d_5pt(256)),
              ("poisson_3d_7pt(32)", problems.poisson_3d_7pt(32))) if args.quick else
             (("poisson_2d_5pt(1024)", problems.poisson_2d_5pt(1024)),
              ("poisson_3d_7pt(128)", problems.poisson_3d_7pt(128))))
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "quick": args.quick,
           "grids": [bench_grid(name, A, args.reps) for name, A in grids]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
