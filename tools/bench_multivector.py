"""Time the multi-vector (n x k) path against k single-vector launches; write profiles/mv/spmm.json.

  python tools/bench_multivector.py [--reps 21] [--out profiles/mv/spmm.json] [--quick]

SpMM: mlamg_spmm for k in {1, 2, 4, 8, 16, 32, 50, 64} on poisson_3d_7pt(128),
poisson_2d_5pt(1024) and random_coeff_3d_7pt(128). Baseline, in the same run: k successive
mlamg_spmv launches on the same handle in the csr_stream format (one column vector each).
Cycle: Hierarchy.cycle_multi against k single Hierarchy.cycle_async calls on a
coarse_format="exact", fine_format="csr_stream" hierarchy.

Timing as the format autotune does (mlamg.autotune.time_format): a warm-up, then per repetition a
cache flush (a 512 MB read), an event, the launches, an event; the median over the repetitions.
The byte model of one SpMM is 12 nnz + 4 (n + 1) + 8 k (n_cols + n_rows); `model_fraction` is
that over 8 TB/s, divided by the measured time.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-amg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

KS = (1, 2, 4, 8, 16, 32, 50, 64)
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


def spmm_model_bytes(A, k):
    return 12.0 * A.nnz + 4.0 * (A.shape[0] + 1) + 8.0 * k * (A.shape[1] + A.shape[0])


def bench_spmm(name, A, reps, flush, ks):
    from mlamg._lib import call, ptr, stream_ptr
    from mlamg.sparse import DeviceCSR
    Ad = DeviceCSR.from_scipy(A).set_format("csr_stream")
    n_rows, n_cols = A.shape
    rows = []
    for k in ks:
        X = torch.randn((n_cols, k), dtype=torch.float64, device="cuda")
        Y = torch.empty((n_rows, k), dtype=torch.float64, device="cuda")
        xs = torch.randn((k, n_cols), dtype=torch.float64, device="cuda")  # one vector per row
        ys = torch.empty((k, n_rows), dtype=torch.float64, device="cuda")
        s = stream_ptr()

        def multi():
            call("mlamg_spmm", Ad.handle, ptr(X), k, ptr(Y), k, k, 1.0, 0.0, s)

        def singles():
            for j in range(k):
                call("mlamg_spmv", Ad.handle, ptr(xs[j]), ptr(ys[j]), 1.0, 0.0, s)

        t_mv = timed_us(multi, reps, flush)
        t_1 = timed_us(singles, reps, flush)
        model = spmm_model_bytes(A, k)
        rows.append({"k": k, "spmm_us": round(t_mv, 2), "k_spmv_us": round(t_1, 2),
                     "speedup": round(t_1 / t_mv, 3), "model_bytes": model,
                     "model_fraction": round(model / PEAK_BPS / (t_mv * 1e-6), 4)})
        print(f"{name:24s} k={k:2d}  spmm {t_mv:9.1f} us   {k} x spmv {t_1:9.1f} us   "
              f"x{t_1 / t_mv:5.2f}   {rows[-1]['model_fraction']:.3f} of model", flush=True)
        del X, Y, xs, ys
    return {"matrix": name, "n_rows": n_rows, "n_cols": n_cols, "nnz": int(A.nnz), "k": rows}


def bench_cycle(name, A, reps, flush, ks):
    from mlamg.hierarchy import Hierarchy
    H = Hierarchy.build(A, fine_format="csr_stream", coarse_format="exact")
    n = A.shape[0]
    rows = []
    for k in ks:
        B = torch.randn((n, k), dtype=torch.float64, device="cuda")
        X = torch.zeros((n, k), dtype=torch.float64, device="cuda")
        b = B[:, 0].contiguous()
        x = torch.zeros(n, dtype=torch.float64, device="cuda")

        def multi():
            H.cycle_multi(B, X, 1, history=False)

        def singles():
            for _ in range(k):
                H.cycle_async(b, x, 1, zero_rhs=False)

        t_mv = timed_us(multi, reps, flush)
        t_1 = timed_us(singles, reps, flush)
        rows.append({"k": k, "cycle_multi_us": round(t_mv, 1), "k_cycles_us": round(t_1, 1),
                     "speedup": round(t_1 / t_mv, 3)})
        print(f"cycle {name:18s} k={k:2d}  multi {t_mv:9.1f} us   {k} x cycle {t_1:9.1f} us   "
              f"x{t_1 / t_mv:5.2f}", flush=True)
        del B, X
    return {"matrix": name, "n_rows": n, "levels": H.n_levels, "k": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "spmm.json"))
    ap.add_argument("--quick", action="store_true", help="small matrices (a functional check)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    if a.reps < 20:
        print("note: fewer than 20 repetitions", file=sys.stderr)
    from mlamg import problems
    m3, m2 = (32, 128) if a.quick else (128, 1024)
    mats = ((f"poisson_3d_7pt({m3})", lambda: problems.poisson_3d_7pt(m3)),
            (f"poisson_2d_5pt({m2})", lambda: problems.poisson_2d_5pt(m2)),
            (f"random_coeff_3d_7pt({m3})", lambda: problems.random_coeff_3d_7pt(m3)))
    flush = torch.ones((512 << 20) // 8, dtype=torch.float64, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "peak_bytes_per_s": PEAK_BPS,
           "timing": "median of reps launches, each after a 512 MB cache-flushing read; "
                     "stream events around the launches",
           "baseline": "k successive mlamg_spmv launches, csr_stream format, same handle",
           "spmm": [], "cycle": []}
    for name, make in mats:
        A = make().tocsr()
        res["spmm"].append(bench_spmm(name, A, a.reps, flush, KS))
    A = problems.poisson_2d_5pt(m2).tocsr()
    res["cycle"].append(bench_cycle(f"poisson_2d_5pt({m2})", A, a.reps, flush, (1, 8, 32)))
    res["k8_faster_everywhere"] = all(r["speedup"] > 1.0 for m in res["spmm"] for r in m["k"]
                                      if r["k"] == 8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)
    return 0 if res["k8_faster_everywhere"] else 1


if __name__ == "__main__":
    sys.exit(main())
