"""Time the block GMRES against successive single solves; write profiles/mv/block_gmres.json.

  python tools/bench_block_gmres.py [--reps 11] [--out profiles/mv/block_gmres.json] [--quick]

Problems, both on poisson_2d_5pt(1024) (1,048,576 rows):
  build      Hierarchy.build(A): weighted-Jacobi levels, dense coarse solve
  pyamg_sa   Hierarchy.pyamg_sa(A) after enable_block_gauss_seidel(): symmetric Gauss-Seidel on
             every level (the block sweep)

For k in {1, 8, 32}: one mlamg_gmres_mv on k random right-hand sides against k successive
mlamg_gmres calls on the same hierarchy and the same right-hand sides, in the same run (rtol 1e-8,
restart 20, zero initial guess, no history): median of --reps between stream events around the
call(s), the zeroing of the iterate included on both sides (the host reads one status per Krylov
step inside, so the interval is the time from the first launch to the end of the last one). The
step counts per column are recorded, and every column is compared bit for bit.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-amg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

KS = (1, 8, 32)
RTOL, RESTART, MAXITER = 1e-8, 20, 100


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


def bench(H, reps):
    from mlamg._lib import call, ptr, stream_ptr
    A = H.levels[0].A
    n = A.shape[0]
    rows = []
    for k in KS:
        g = torch.Generator(device="cuda").manual_seed(300 + k)
        B = torch.randn((n, k), dtype=torch.float64, device="cuda", generator=g)
        X = torch.zeros_like(B)
        cols = [B[:, j].contiguous() for j in range(k)]
        xs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(k)]
        s = stream_ptr()
        info_b, it_b = (ctypes.c_int32 * k)(), (ctypes.c_int32 * k)()
        info_s, it_s = [ctypes.c_int() for _ in range(k)], [ctypes.c_int() for _ in range(k)]

        def block():
            X.zero_()
            call("mlamg_gmres_mv", A.handle, H.handle, ptr(B), k, ptr(X), k, k, RTOL, RESTART,
                 MAXITER, 1, info_b, it_b, None, 0, s)

        def singles():
            for j in range(k):
                xs[j].zero_()
                call("mlamg_gmres", A.handle, H.handle, ptr(cols[j]), ptr(xs[j]), RTOL, RESTART,
                     MAXITER, 1, ctypes.byref(info_s[j]), ctypes.byref(it_s[j]), None, 0, s)

        t_block = event_ms(block, reps)
        t_single = event_ms(singles, reps)
        H.check_coarse()
        same = (all(torch.equal(X[:, j], xs[j]) for j in range(k))
                and list(it_b) == [v.value for v in it_s]
                and list(info_b) == [v.value for v in info_s])
        row = {"k": k, "block_ms": round(t_block, 3), "k_single_solves_ms": round(t_single, 3),
               "speedup": round(t_single / t_block, 3), "steps_per_column": list(it_b),
               "info_per_column": list(info_b), "columns_bitwise_equal": bool(same)}
        rows.append(row)
        print(f"k={k:2d}  block {t_block:9.3f} ms   {k} single solves {t_single:9.3f} ms   "
              f"x{t_single / t_block:5.2f}   steps {sorted(set(it_b))}  bitwise {same}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "block_gmres.json"))
    ap.add_argument("--quick", action="store_true", help="a small grid (a functional check)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    m = 128 if a.quick else 1024
    A = problems.poisson_2d_5pt(m).tocsr()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "problem": f"poisson_2d_5pt({m})", "n": A.shape[0], "rtol": RTOL, "restart": RESTART,
           "timing": "median of reps between stream events around the call(s), zeroing of the "
                     "iterate included",
           "hierarchies": []}
    for name in ("build", "pyamg_sa"):
        if name == "build":
            H = Hierarchy.build(A)
            if any(f[0] == "vector" for lv in H.formats() for f in lv.values()):
                H.enable_block_vector()
        else:
            H = Hierarchy.pyamg_sa(A).enable_block_gauss_seidel()
        print(f"{name}: {H.n_levels} levels", flush=True)
        res["hierarchies"].append({"hierarchy": name, "levels": H.n_levels, "k": bench(H, a.reps)})
        del H
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
