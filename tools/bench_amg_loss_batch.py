"""Time AmgLossBatch against a loop of single amg_loss_and_grad calls; write
profiles/mv/amg_loss_batch.json.

  python tools/bench_amg_loss_batch.py [--reps 7] [--loop-reps 3] [--out FILE] [--quick]
  python tools/bench_amg_loss_batch.py --single-only --out FILE     (runs on any older tree)

Problems: poisson_2d_5pt(m) with m cycling over 16, 24, 32, 48, 3 x 3 box aggregates (coarse
blocks of 36, 64, 121 and 256 rows) and the smoothed prolongator P = (I - 2/3 D^-1 A) Agg; seeded
unit test vectors. For nb in {16, 64, 256}, k in {8, 50} and tot_num_loop in {5, 20}:
  batch_ms    median wall time of one AmgLossBatch.loss_and_grad step on an object built
              beforehand (device idle before and after), and its phases (a separate profiled run
              that synchronises between them): upload + Galerkin, block inverse, forward, backward
  loop_ms     median wall time of the loop of nb amg_loss_and_grad calls on the same problems
              (scipy operators and host test vectors given, as a training loop holds them). The
              loop uses only functions that exist unchanged before the batch was added, so
              --single-only measures the same thing on an older tree.
And, on the coarse operators of the nb problems: one mlamg_blockdense_create on their stack against
nb mlamg_dense_create calls, with the library's method rule and with Gauss-Jordan forced for every
block (MLAMG_DENSE_GJ)."""
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

MS = (16, 24, 32, 48)


def problem(m, k):
    from mlamg import problems
    A = problems.poisson_2d_5pt(m).tocsr().astype(np.float64)
    A.sort_indices()
    n = A.shape[0]
    agg = sp.csr_matrix(problems.box_aggregates_2d(m, m, 3))
    Dinv = sp.diags([1.0 / A.diagonal()], [0])
    P = sp.csr_matrix((sp.eye(n) - (2.0 / 3.0) * Dinv @ A) @ agg)
    P.sum_duplicates()
    P.sort_indices()
    X = np.random.RandomState(m).standard_normal((n, k))
    return A, P, X / np.linalg.norm(X, 2, axis=0)


def wall_ms(fn, reps):
    """Median wall time (ms) of fn() over reps calls after one warm-up, device idle before and
    after each."""
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def bench_inverse(probs, reps):
    """One block-diagonal inverse against nb single ones, on the problems' coarse operators."""
    from mlamg._lib import call, lib, stream_ptr
    from mlamg.loss import BlockDense
    from mlamg.sparse import DeviceCSR
    Acs = [sp.csr_matrix(P.T @ A @ P) for A, P, _ in probs]
    off = np.concatenate([[0], np.cumsum([a.shape[0] for a in Acs])]).astype(np.int64)
    stack = DeviceCSR.from_scipy(sp.block_diag(Acs, format="csr"))
    singles = [DeviceCSR.from_scipy(a) for a in Acs]

    def batched():
        BlockDense(stack, off)

    def looped():
        for a in singles:
            h = ctypes.c_void_p()
            call("mlamg_dense_create", a.handle, ctypes.byref(h), stream_ptr())
            lib.mlamg_dense_destroy(h)

    out = {}
    for name, gj in (("method_rule", False), ("gauss_jordan_forced", True)):
        if gj:
            os.environ["MLAMG_DENSE_GJ"] = "1"
        try:
            methods = BlockDense(stack, off).methods()
            b = wall_ms(batched, reps)
            s = wall_ms(looped, max(2, reps // 2))
        finally:
            os.environ.pop("MLAMG_DENSE_GJ", None)
        out[name] = {"blockdense_create_ms": round(b[0], 3), "dense_create_loop_ms": round(s[0], 3),
                     "loop_over_batch": round(s[0] / b[0], 2),
                     "gauss_jordan_blocks": methods.count(0), "cholesky_blocks": methods.count(1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "amg_loss_batch.json"))
    ap.add_argument("--quick", action="store_true", help="nb = 8 only (a functional check)")
    ap.add_argument("--single-only", action="store_true",
                    help="only the loop of single calls (runs on a tree without the batch)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from mlamg import loss
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "loop_reps": a.loop_reps,
           "single_only": bool(a.single_only),
           "timing": "median wall time (ms) of the step / the loop, device idle before and after; "
                     "phases: a separate run of the step that synchronises between phases",
           "problems": "poisson_2d_5pt(m), m cycling over 16, 24, 32, 48; 3x3 boxes; V(1,1)",
           "rows": [], "inverse": []}
    for nb in ((8,) if a.quick else (16, 64, 256)):
        for k in (8, 50):
            base = {m: problem(m, k) for m in MS}
            probs = [base[MS[i % len(MS)]] for i in range(nb)]
            As, Ps, Xs = (list(t) for t in zip(*probs))
            if k == 8 and not a.single_only:
                inv = bench_inverse(probs, a.reps)
                inv["nb"] = nb
                res["inverse"].append(inv)
                print("inverse", json.dumps(inv), flush=True)
            for T in (5, 20):
                row = {"nb": nb, "k": k, "tot_num_loop": T, "rows_total": sum(A.shape[0] for A in As)}

                def loop():
                    for A, P, X in probs:
                        loss.amg_loss_and_grad(P, A, X, T)

                med, lo, hi = wall_ms(loop, a.loop_reps)
                row.update(loop_ms=round(med, 2), loop_ms_min=round(lo, 2), loop_ms_max=round(hi, 2))
                if not a.single_only:
                    B = loss.AmgLossBatch(As, Ps, Xs, T)
                    values = np.concatenate([P.data for P in Ps])
                    med, lo, hi = wall_ms(lambda: B.loss_and_grad(values), a.reps)
                    row.update(batch_ms=round(med, 3), batch_ms_min=round(lo, 3),
                               batch_ms_max=round(hi, 3), loop_over_batch=round(row["loop_ms"] / med, 2))
                    B.profile = True
                    ph = []
                    for _ in range(max(3, a.reps // 2)):
                        B.loss_and_grad(values)
                        ph.append(dict(B.phases))
                    B.profile = False
                    row["phases_ms"] = {p: round(statistics.median(d[p] for d in ph) * 1e3, 3)
                                        for p in ph[0]}
                    del B
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
