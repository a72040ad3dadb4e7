"""Time the canonical-order SpMM (mlamg_spmm_vec) on the VECTOR-format operators of a default
hierarchy against k single-vector launches; write profiles/mv/spmm_vec.json.

  python tools/bench_spmm_vec.py [--reps 21] [--out profiles/mv/spmm_vec.json] [--quick]

Hierarchy.build(poisson_3d_7pt(128)) with its default formats: the operators the family rule put
in the VECTOR format are listed (shape, nnz, mean row, tuned width), and for each of them and k in
{1, 2, 4, 8, 16, 32, 64} one mlamg_spmm_vec launch is timed against k successive mlamg_spmv
launches on the same handle (VECTOR format active, the tuned width), in the same run, after every
column of the block was checked bitwise against the single launches. mlamg_spmm (scipy's order) on
the same operator is timed beside them: what the canonical order costs. Then the block cycle of
that hierarchy after enable_block_vector() at k = 8 and 32 against k single cycles.

Timing as tools/bench_multivector.py: a warm-up, then per repetition a cache flush (a 512 MB
read), an event, the launches, an event; the median over the repetitions. The byte model of one
launch is (10 or 12) nnz + 4 (n + 1) + 8 k (n_cols + n_rows) — 10 with the 16-bit column copy
(n_cols <= 65536); `model_fraction` is that over 8 TB/s, divided by the measured time.
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

import torch  # noqa: E402

KS = (1, 2, 4, 8, 16, 32, 64)
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


def model_bytes(M, k):
    per_nnz = 10.0 if M.shape[1] <= 65536 else 12.0
    return per_nnz * M.nnz + 4.0 * (M.shape[0] + 1) + 8.0 * k * (M.shape[1] + M.shape[0])


def bench_operator(name, M, reps, flush):
    from mlamg._lib import call, ptr, stream_ptr
    n_rows, n_cols = M.shape
    width = M.get_format()[1]
    rows = []
    for k in KS:
        X = torch.randn((n_cols, k), dtype=torch.float64, device="cuda")
        Y = torch.empty((n_rows, k), dtype=torch.float64, device="cuda")
        xs = X.t().contiguous()  # one vector per row
        ys = torch.empty((k, n_rows), dtype=torch.float64, device="cuda")
        s = stream_ptr()

        def multi():
            call("mlamg_spmm_vec", M.handle, ptr(X), k, ptr(Y), k, k, 1.0, 0.0, s)

        def scipy_order():
            call("mlamg_spmm", M.handle, ptr(X), k, ptr(Y), k, k, 1.0, 0.0, s)

        def singles():
            for j in range(k):
                call("mlamg_spmv", M.handle, ptr(xs[j]), ptr(ys[j]), 1.0, 0.0, s)

        multi()
        singles()
        if not torch.equal(Y.t(), ys):
            raise SystemExit(f"{name} k={k}: mlamg_spmm_vec is not bitwise the single launches")
        t_mv = timed_us(multi, reps, flush)
        t_1 = timed_us(singles, reps, flush)
        t_csr = timed_us(scipy_order, reps, flush)
        model = model_bytes(M, k)
        rows.append({"k": k, "spmm_vec_us": round(t_mv, 2), "k_spmv_us": round(t_1, 2),
                     "speedup": round(t_1 / t_mv, 3), "spmm_scipy_order_us": round(t_csr, 2),
                     "model_bytes": model,
                     "model_fraction": round(model / PEAK_BPS / (t_mv * 1e-6), 4)})
        print(f"{name:4s} k={k:2d}  spmm_vec {t_mv:8.1f} us   {k:2d} x spmv {t_1:8.1f} us   "
              f"x{t_1 / t_mv:5.2f}   {rows[-1]['model_fraction']:.3f} of model   "
              f"(spmm, scipy order {t_csr:8.1f} us)", flush=True)
        del X, Y, xs, ys
    return {"operator": name, "n_rows": n_rows, "n_cols": n_cols, "nnz": int(M.nnz),
            "mean_row": round(M.nnz / max(n_rows, 1), 1), "vec_width": width, "k": rows}


def bench_cycle(H, reps, flush, ks):
    n = H.levels[0].A.shape[0]
    H.enable_block_vector()
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
        print(f"cycle k={k:2d}  multi {t_mv:9.1f} us   {k} x cycle {t_1:9.1f} us   "
              f"x{t_1 / t_mv:5.2f}", flush=True)
        del B, X
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "spmm_vec.json"))
    ap.add_argument("--quick", action="store_true", help="a 48^3 grid (a functional check)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    if a.reps < 20:
        print("note: fewer than 20 repetitions", file=sys.stderr)
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    m = 48 if a.quick else 128
    H = Hierarchy.build(problems.poisson_3d_7pt(m))
    flush = torch.ones((512 << 20) // 8, dtype=torch.float64, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "peak_bytes_per_s": PEAK_BPS,
           "problem": f"Hierarchy.build(poisson_3d_7pt({m})), default formats",
           "levels": H.n_levels,
           "timing": "median of reps launches, each after a 512 MB cache-flushing read; "
                     "stream events around the launches",
           "baseline": "k successive mlamg_spmv launches, VECTOR format at the tuned width, "
                       "same handle",
           "formats": [], "operators": [], "cycle": []}
    for l, L in enumerate(H.levels):
        for tag, M in (("A", L.A), ("P", L.P), ("R", L.R)):
            fmt, width, _ = M.get_format()
            res["formats"].append({"operator": f"{tag}{l}", "shape": list(M.shape),
                                   "nnz": int(M.nnz), "format": fmt,
                                   "vec_width": width if fmt == "vector" else 0})
            if fmt == "vector":
                res["operators"].append(bench_operator(f"{tag}{l}", M, a.reps, flush))
    if not res["operators"]:
        print("no operator of this hierarchy is in the VECTOR format", file=sys.stderr)
    res["cycle"] = bench_cycle(H, a.reps, flush, (8, 32))
    k8 = [r["speedup"] for op in res["operators"] for r in op["k"] if r["k"] == 8]
    res["k8_faster_everywhere"] = bool(k8) and all(v > 1.0 for v in k8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
