"""Time the block Gauss-Seidel sweep (mlamg_gs_sweep_mv) against k single sweeps,
and the block V-cycle with Gauss-Seidel levels against k single cycles; write
profiles/mv/block_gs.json.

  python tools/bench_block_gs.py [--reps 21] [--out profiles/mv/block_gs.json] [--quick]

Sweeps: one mlamg_gs_sweep_mv on an (n, k) block against k successive mlamg_gs_sweep launches on
the same handle in the same run (the single-vector code is the baseline), k in {1, 2, 4, 8, 16,
32, 64}, on poisson_2d_5pt(256), poisson_2d_5pt(1024), poisson_3d_7pt(64) (forward
gauss_seidel handles) and level 1 of Hierarchy.pyamg_sa(poisson_2d_5pt(256)) (its symmetric
block Gauss-Seidel handle: long rows, the walk on the CSR arrays). Every block column is checked
bitwise against its single sweep before anything is timed, and the path that ran is recorded.

Crossover: every k is also timed with the selection forced each way (MLAMG_GS_MV_WALK_ITEMS:
0 = one launch per level, a huge value = the one-workgroup walk); the walk's passes over its
widest level are ceil(max_level_rows * ceil(k / 2) / 1024).

Cycle: the block cycle of pyamg_sa(poisson_2d_5pt(1024)) with enable_block_gauss_seidel() at
k = 8 and 32 against k single cycles.

Timing: a warm-up, then medians over `reps` repetitions, stream events around the launches.
Nothing is gated on a ratio."""
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
PATHS = {0: "per_level", 1: "walk_csr", 2: "walk_packed"}


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


def forced(items):
    """Context: the selection constant replaced (None: the built-in rule)."""
    class _F:
        def __enter__(self):
            if items is None:
                os.environ.pop("MLAMG_GS_MV_WALK_ITEMS", None)
            else:
                os.environ["MLAMG_GS_MV_WALK_ITEMS"] = str(items)

        def __exit__(self, *exc):
            os.environ.pop("MLAMG_GS_MV_WALK_ITEMS", None)
    return _F()


def bench_sweep(name, gs, n, reps, ks, crossover):
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(5)
    for k in ks:
        X0 = torch.randn((n, k), dtype=torch.float64, device="cuda", generator=gen)
        B = torch.randn((n, k), dtype=torch.float64, device="cuda", generator=gen)
        x0s = X0.t().contiguous()  # one vector per row
        bs = B.t().contiguous()
        # bitwise: every block column against its single sweep, on every path that is timed
        ref = x0s.clone()
        for j in range(k):
            gs.sweep(ref[j], bs[j], 1)
        for items in ((None, 0, 1 << 40) if crossover else (None,)):
            with forced(items):
                X = X0.clone()
                gs.sweep(X, B, 1)
            assert torch.equal(X.t(), ref), (name, k, items)
        X = X0.clone()
        xs = x0s.clone()

        def multi():
            gs.sweep(X, B, 1)

        def singles():
            for j in range(k):
                gs.sweep(xs[j], bs[j], 1)

        path = gs.mv_path(k)
        t_mv = timed_us(multi, reps)
        t_1 = timed_us(singles, reps)
        row = {"k": k, "path": PATHS[path], "sweep_mv_us": round(t_mv, 1),
               "k_sweeps_us": round(t_1, 1), "speedup": round(t_1 / t_mv, 3),
               "us_per_level": round(t_mv / gs.n_levels, 3)}
        if crossover:
            with forced(0):
                row["forced_per_level_us"] = round(timed_us(multi, reps), 1)
            with forced(1 << 40):
                row["forced_walk_us"] = round(timed_us(multi, reps), 1)
        rows.append(row)
        print(f"{name:34s} k={k:2d} {PATHS[path]:11s} block {t_mv:9.1f} us   {k} x single "
              f"{t_1:9.1f} us   x{t_1 / t_mv:5.2f}"
              + (f"   forced: per-level {row['forced_per_level_us']:9.1f}  walk "
                 f"{row['forced_walk_us']:9.1f}" if crossover else ""), flush=True)
        del X0, B, x0s, bs, ref, X, xs
    return {"problem": name, "n": n, "levels": gs.n_levels, "k": rows}


def bench_cycle(name, H, reps, ks):
    n = H.levels[0].A.shape[0]
    H.enable_block_gauss_seidel()
    rows = []
    for k in ks:
        B = torch.randn((n, k), dtype=torch.float64, device="cuda")
        X = torch.zeros((n, k), dtype=torch.float64, device="cuda")
        b = B[:, 0].contiguous()
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        Z = H.precondition(B)  # bitwise: column 0 against the single cycle
        assert torch.equal(Z[:, 0], H.precondition(b)), (name, k)

        def multi():
            H.cycle_multi(B, X, 1, history=False)

        def singles():
            for _ in range(k):
                H.cycle(b, x, 1, use_graph=False, history=False)

        t_mv = timed_us(multi, reps)
        t_1 = timed_us(singles, reps)
        rows.append({"k": k, "cycle_multi_us": round(t_mv, 1), "k_cycles_us": round(t_1, 1),
                     "speedup": round(t_1 / t_mv, 3)})
        print(f"cycle {name:28s} k={k:2d}  block {t_mv:10.1f} us   {k} x cycle {t_1:10.1f} us   "
              f"x{t_1 / t_mv:5.2f}", flush=True)
        del B, X, Z
    return {"problem": name, "n": n, "levels": H.n_levels, "k": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "block_gs.json"))
    ap.add_argument("--quick", action="store_true", help="small problems (a functional check)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    from mlamg.multigrid import GaussSeidel
    from mlamg.sparse import DeviceCSR
    ma, mb, m3 = (48, 96, 16) if a.quick else (256, 1024, 64)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "timing": "median of reps repetitions after a warm-up; stream events around the "
                     "launches",
           "baseline": "k successive mlamg_gs_sweep launches (k single cycles), same handle, "
                       "same run",
           "sweep": [], "cycle": []}
    keep = []
    for name, make, cross in ((f"poisson_2d_5pt({ma})", lambda: problems.poisson_2d_5pt(ma), True),
                              (f"poisson_2d_5pt({mb})", lambda: problems.poisson_2d_5pt(mb), True),
                              (f"poisson_3d_7pt({m3})", lambda: problems.poisson_3d_7pt(m3), True)):
        Ad = DeviceCSR.from_scipy(make().tocsr())
        gs = GaussSeidel(Ad)
        keep.append((Ad, gs))
        res["sweep"].append(bench_sweep(name, gs, Ad.shape[0], a.reps, KS, cross))
    Hs = Hierarchy.pyamg_sa(problems.poisson_2d_5pt(ma))
    L1 = Hs.levels[1]
    res["sweep"].append(bench_sweep(f"pyamg_sa(poisson_2d_5pt({ma})) level 1", L1.gs,
                                    L1.A.shape[0], a.reps, KS, True))
    Hc = Hierarchy.pyamg_sa(problems.poisson_2d_5pt(mb))
    res["cycle"].append(bench_cycle(f"pyamg_sa(poisson_2d_5pt({mb}))", Hc, a.reps, (8, 32)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
