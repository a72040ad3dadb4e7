"""Benchmark: V-cycles/sec of the MI355X AMG V-cycle on the 3D 7-point Laplace 216^3 (C4).

One step = one multilevel weighted-Jacobi V(1,1)-cycle (the MLAMG.amg_2_v cycle of
ns/preconditioner/MLAMG.py:189-195, applied recursively) over the whole 10,077,696-DoF problem,
including the end-of-cycle residual norm (MLAMG.py:194). Setup (aggregation, lambda_max, SA
prolongators, Galerkin, dense coarse inverse) runs on the GPU before timing and is reported
separately.

  python bench.py [--gpus N --steps K --warmup W] [--n 216] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line. --dump-outputs DIR
then writes what the last timed step left in the caller's hands (the iterate x) as DIR/x.npy.
--full adds every other measurement to the line: the convergence sample, the general-b and
factored-P0 cycles, the fine-SpMV roofline and format A/B, the PCIe-inclusive solve, the
unstructured (C3) and variable-coefficient lines and the CPU baselines.

N > 1: one process per GPU — launched by torch.distributed.run (RANK/WORLD_SIZE/... in the
environment), or, when started as plain `python bench.py --gpus N`, by bench.py itself: it
starts N ranks as child processes with the same environment torch.distributed.run would give
them (before anything touches the GPU) and exits with their status. Every level with at least
--dist-min-rows rows is row-partitioned (contiguous slabs; coarse rows follow their aggregate
seed) with RCCL halo exchanges, the coarser levels are replicated (mlamg.distributed).
Rank 0 prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "ml-amg_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

METRIC = "V-cycles/sec + fine-level SpMV GB/s (%HBM peak), 3D Laplace 10M DoF"
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)


DUMP_MAX_BYTES = 32 << 20  # per dumped array; larger outputs are sampled
DUMP_SEED = 20240607


def dump_array(a):
    """The array --dump-outputs stores for output `a` (flattened, float32 kept, everything else
    float64): `a` itself up to DUMP_MAX_BYTES, otherwise its entries at DUMP_MAX_BYTES / itemsize
    positions drawn once from RandomState(DUMP_SEED) without replacement, in ascending order —
    the same positions for the same length, so two builds are compared entry for entry."""
    a = np.asarray(a)
    a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64).ravel()
    keep = DUMP_MAX_BYTES // a.itemsize
    if a.size <= keep:
        return a
    idx = np.sort(np.random.RandomState(DUMP_SEED).choice(a.size, size=keep, replace=False))
    return a[idx]


def dump_outputs(dirname, arrays):
    """--dump-outputs: one DIR/<name>.npy per output of the timed path."""
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), dump_array(a))


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


def host_cores():
    """(threads, description): the host CPUs this process may run on — the affinity mask
    (os.sched_getaffinity; os.cpu_count() ignores it) capped by the cgroup CPU quota
    (/sys/fs/cgroup/cpu.max), which is what bounds a parallel CPU baseline here."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, period = fh.read().split()[:2]
        if q != "max":
            quota = max(1, int(float(q) / float(period)))
    except (OSError, ValueError):
        pass
    threads = min(aff, quota) if quota else aff
    desc = (f"affinity {aff} CPUs, cgroup quota {quota if quota else 'none'}, "
            f"machine nproc {os.cpu_count()}")
    return threads, desc


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n, argv):
    """`python bench.py --gpus N` with no launcher around it: start N ranks of this script as
    child processes, each with the environment torch.distributed.run gives a rank (RANK,
    LOCAL_RANK, WORLD_SIZE, LOCAL_WORLD_SIZE, MASTER_ADDR=127.0.0.1, MASTER_PORT). This process
    never touches the GPU. Rank 0's stdout (the JSON line) is inherited. If a rank fails the
    others are stopped (by their own PIDs) and its status is returned."""
    import subprocess
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), GROUP_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv,
                                      env=env))
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in live:
                    q.terminate()
        if live:
            time.sleep(0.2)
    return rc if rc >= 0 else 128 - rc


def launch_selftest(world, rank):
    """--launch-selftest: rendezvous of the launched ranks over gloo (no GPU), rank 0 prints
    what every rank saw — proves the self-launch starts N ranks with a consistent environment."""
    import torch.distributed as dist
    if os.environ.get("MLAMG_SELFTEST_FAIL_RANK") == str(rank):
        raise SystemExit(3)  # test hook: a rank that dies before the rendezvous
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(_free_port()))
    dist.init_process_group("gloo", world_size=world, rank=rank)
    mine = {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "-1")),
            "world": world, "pid": os.getpid(),
            "master": f"{os.environ.get('MASTER_ADDR')}:{os.environ.get('MASTER_PORT')}"}
    seen = [None] * world
    dist.all_gather_object(seen, mine)
    if rank == 0:
        print(json.dumps({"launch_selftest": True, "n_gpus": world, "ranks": seen}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def spmv_bytes(n_rows, n_cols, nnz):
    """12*nnz + 4*(n+1) + 8*n_cols (x) + 8*n (y)."""
    return 12.0 * nnz + 4.0 * (n_rows + 1) + 8.0 * n_cols + 8.0 * n_rows


def aggregation_rule(args):
    """The aggregation rule a bench line used, in words (config.workload)."""
    if args.aggregation == "reference":
        order = ("columns relabelled in ascending seed order" if args.coarse_order == "sorted"
                 else "nearest_center_to_agg column order")
        return ("level 0: the reference's push-order modified_bellman_ford from unsorted "
                f"RandomState(0) seeds, graph.py:40-51, {order}; coarser levels: "
                "order-independent rule, sorted seeds")
    return "every level: order-independent rule (smallest tight seed), sorted seeds"


def time_kernel(fn, reps=50):
    """mlamg.timing.time_kernel (imported lazily: the self-launching parent never loads HIP)."""
    from mlamg.timing import time_kernel as tk
    return tk(fn, reps)


def time_kernel_cold(fn, reps=20):
    """mlamg.timing.time_kernel_cold: cold launches timed by their own dispatch packet."""
    from mlamg.timing import time_kernel_cold as tkc
    return tkc(fn, reps)


def load_traffic(name):
    """HBM bytes per launch of the dominant kernel measured with rocprofv3 --pmc
    (profiles/*_pmc.json written by tools/pmc_traffic.py), or None."""
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None
    try:
        with open(path) as fh:
            return json.load(fh)
    except Exception:
        return None


def cpu_baseline(H, b_host, x_host, cycles):
    """Oracle (scipy restatement of the reference cycle) on the same hierarchy, 1 thread."""
    from threadpoolctl import threadpool_limits
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from oracle import restated as orc

    levels = []
    for L in H.levels:
        A = L.A.to_scipy()
        levels.append({"A": A, "P": L.P.to_scipy(), "Dw": sp.diags(L.dinv.cpu().numpy())})
    Ac = H.Ac.to_scipy()
    with threadpool_limits(limits=1):
        lu = spla.factorized(sp.csc_matrix(Ac))
        # one untimed cycle (page in), then the timed sample
        orc.vcycle_solve(levels, Ac, b_host, x_host, 1, lu=lu)
        t0 = time.perf_counter()
        _, hist = orc.vcycle_solve(levels, Ac, b_host, x_host, cycles, lu=lu)
        dt = time.perf_counter() - t0
    return cycles / dt, dt, hist


def cpu_baseline_parallel(H, b_host, x_host, cycles, threads):
    """BASELINE ONLY: the same cycle with OpenMP row-parallel CSR kernels (oracle/omp_cycle.c) on
    `threads` host threads, coarse solve by the dense inverse (as the device)."""
    from oracle import restated as orc

    levels = [{"A": L.A.to_scipy(), "P": L.P.to_scipy(), "d": L.dinv.cpu().numpy()}
              for L in H.levels]
    Ainv = np.linalg.inv(H.Ac.to_scipy().toarray())
    orc.vcycle_omp(levels, Ainv, b_host, x_host, 1, threads)  # page in
    t0 = time.perf_counter()
    _, hist = orc.vcycle_omp(levels, Ainv, b_host, x_host, cycles, threads)
    dt = time.perf_counter() - t0
    return cycles / dt, dt, hist


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", "--grid", dest="n", type=int, default=216,
                    help="grid points per dimension (C4: 216); use --grid under torchrun")
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--max-coarse", type=int, default=2000)
    ap.add_argument("--aggregation", choices=("reference", "bellman_ford"), default="reference",
                    help="level-0 aggregates: 'reference' = the reference's push-order seeded "
                         "Bellman-Ford (ns/lib/graph.py:40-51, utils/evaluate_dataset.py:80-90); "
                         "'bellman_ford' = the order-independent rule on every level")
    ap.add_argument("--coarse-order", choices=("sorted", "seed"), default="sorted",
                    help="aggregation='reference': level-0 coarse unknowns in ascending seed "
                         "order (same aggregates, relabelled) or nearest_center_to_agg's order")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline, run every other measurement and check of the "
                         "benchmark (convergence sample, general-b and factored-P0 cycles, "
                         "fine-SpMV roofline and format A/B, PCIe-inclusive solve, C3 and "
                         "variable-coefficient lines, CPU baselines); off: the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last of them computed (the "
                         "iterate x the caller's buffer holds) as DIR/x.npy (float64; a fixed "
                         "seeded sample of its entries when x is larger than "
                         f"{DUMP_MAX_BYTES >> 20} MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-cycles", type=int, default=20)
    ap.add_argument("--cpu-par-cycles", type=int, default=10)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--dist", action="store_true",
                    help="use the distributed executor even at N=1 (tests the RCCL path)")
    ap.add_argument("--dist-min-rows", type=int, default=50000,
                    help="distributed run: row-partition every level with at least this many "
                         "rows (the rest are replicated on each GPU)")
    ap.add_argument("--dist-setup", action="store_true",
                    help="distributed run: build the partitioned levels with the distributed "
                         "setup (mlamg.dsetup: each rank its rows; SURVEY.md §8(e)) instead of "
                         "replicating the whole hierarchy on every rank")
    ap.add_argument("--overlap-min-rows", type=int, default=2_000_000,
                    help="distributed run: split local operators of at least this many rows so "
                         "their halo exchange overlaps the interior rows (-1: never)")
    ap.add_argument("--no-c3", action="store_true",
                    help="skip the unstructured (C3) fine-SpMV roofline line")
    ap.add_argument("--no-varcoef", action="store_true",
                    help="skip the variable-coefficient 216^3 cycle beside the headline")
    ap.add_argument("--launch-selftest", action="store_true",
                    help="launch the ranks, rendezvous over gloo and report them; no GPU work")
    ap.add_argument("--phase-selftest", action="store_true",
                    help="run the distributed phase sequence over gloo with its watchdog (a "
                         "stall injected by MLAMG_STALL_RANK_PHASE=rank:phase); no GPU work")
    ap.add_argument("--verify-selftest", action="store_true",
                    help="run the distributed verification chain over gloo (mismatch injected "
                         "by MLAMG_INJECT_MISMATCH_RANK); no GPU work")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and (args.gpus > 1 or args.dist):
        ap.error("--dump-outputs is for the single-GPU run (no --dist, --gpus 1)")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # plain `python bench.py --gpus N`: become the launcher (nothing has touched the GPU)
        sys.exit(self_launch(args.gpus, sys.argv[1:] if argv is None else list(argv)))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus={args.gpus}")
    if args.launch_selftest:
        return launch_selftest(world, rank)
    if args.verify_selftest:
        return verify_selftest(world, rank)
    if args.phase_selftest:
        from mlamg import distributed
        return distributed.phase_selftest(world, rank)
    if os.environ.get("MLAMG_ONE_DEVICE") == "1":
        local_rank = 0  # rehearsal only: every rank on GPU 0 (checks the RCCL code path on 1 GPU)
    torch.cuda.set_device(local_rank)
    if world > 1 or args.dist:
        return run_distributed(args, world, rank, local_rank)

    from mlamg import problems
    from mlamg.hierarchy import Hierarchy

    n1 = args.n
    t0 = time.perf_counter()
    A = problems.poisson_3d_7pt(n1)
    log(f"C4 matrix {A.shape[0]} rows, {A.nnz} nnz built in {time.perf_counter() - t0:.1f}s")
    H = Hierarchy.build(A, alpha=args.alpha, strength_mode="invabs", max_coarse=args.max_coarse,
                        verbose=args.verbose, aggregation=args.aggregation,
                        coarse_order=args.coarse_order)
    setup_s = H.timings["total"]
    for row in H.describe():
        log(row)
    n = A.shape[0]
    x0 = np.random.RandomState(0).randn(n)
    x0 /= np.linalg.norm(x0)
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    x = torch.as_tensor(x0).cuda()
    use_graph = not args.no_graph
    hist = conv = None
    if args.full:
        # convergence sample (also warms the graph)
        hist = H.cycle(b, x, 10, use_graph=use_graph)
        conv = float((hist[-1] / hist[-4]) ** (1.0 / 3.0)) if len(hist) >= 4 else float("nan")
        log(f"residual history (10 cycles): {hist[0]:.3e} -> {hist[-1]:.3e}, "
            f"conv factor {conv:.4f}")
    else:
        # one untimed cycle: the graph capture and first launches happen here, not in a step
        H.cycle_async(b, x, 1, use_graph=use_graph)
    x.copy_(torch.as_tensor(x0))
    H.cycle_async(b, x, args.warmup, use_graph=use_graph)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    H.cycle_async(b, x, args.steps, use_graph=use_graph)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cycles_per_s = args.steps / dt
    ms_per_step = dt / args.steps * 1e3
    if args.dump_outputs:
        # the timed call's only output: the iterate it left in the caller's x
        dump_outputs(args.dump_outputs, {"x": x.cpu().numpy()})
    A0 = H.levels[0].A
    cyc_bytes = H.cycle_bytes()                # operators priced as CSR (§8(d)), the timed b
    cyc_fmt_bytes = H.cycle_bytes(stored=True)  # operators priced as stored: HBM bytes
    t_cycle = dt / args.steps
    out = {
        "metric": METRIC,
        "value": round(cycles_per_s, 3),
        "unit": "V-cycles/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": f"C4: 3D 7-point Laplace {n1}^3 ({n} DoF, nnz {A0.nnz}), SA-AMG "
                        f"V(1,1) weighted Jacobi w=2/3, seeded Bellman-Ford aggregates "
                        f"alpha={args.alpha} ({aggregation_rule(args)}), {H.n_levels} levels, "
                        f"dense coarse n={H.Ac.shape[0]}",
                "aggregation": args.aggregation, "coarse_order": args.coarse_order,
            "n": n, "nnz": A0.nnz, "levels": H.n_levels,
            "operator_complexity": round(H.operator_complexity(), 4),
            "parallelism": "single GPU",
        },
        # whole cycle: the bytes its launches must move as stored (every operator's format
        # bytes + the epilogue vectors) over the cycle time = the cycle's HBM fraction; the
        # CSR-priced figure is a CSR-EQUIVALENT rate (re-encoded operators move fewer bytes,
        # so it can exceed the peak) and is labelled as such
        "cycle_format_bytes": cyc_fmt_bytes,
        "cycle_hbm_GBps": round(cyc_fmt_bytes / t_cycle / 1e9, 1),
        "cycle_hbm_frac": round(cyc_fmt_bytes / t_cycle / 1e9 / HBM_PEAK_GBPS, 4),
        "cycle_csr_bytes": cyc_bytes,
        "cycle_csr_equivalent_GBps": round(cyc_bytes / t_cycle / 1e9, 1),
        "operator_formats": [{k: v[0] + (f"/{v[1]}" if v[1] else "") for k, v in f.items()}
                             for f in H.formats()],
        "format_autotune_us": H.tuning,
        "setup_s": {k: round(v, 3) for k, v in H.timings.items()},
        "setup_galerkin_s_per_level": H.galerkin_s,
        "setup_spgemm_phases_ms": H.spgemm_phases_ms,
        "rhs": "b = 0 (x0 = RandomState(0).randn normalised): passed to the cycle as NULL, the "
               "fine-level kernels read no b vector (same bits as streaming zeros)",
    }
    if args.full:
        full_lines(out, args, H, A, b, x, x0, hist, conv, use_graph)
    print(json.dumps(out), flush=True)


def full_lines(out, args, H, A, b, x, x0, hist, conv, use_graph):
    """--full: every measurement and check beside the headline, each a run of its own after the
    timed steps, added to the result line `out`."""
    n = A.shape[0]
    # the same cycles with b streamed as a vector (the general right-hand-side kernels): the
    # headline's b is zero (b = 0, utils/common.py:74), which the cycle takes
    # as NULL (hierarchy.rhs_arg) and never reads — identical bits (tests/test_gpu_hierarchy.py
    # test_zero_rhs_same_bits); this line shows what a nonzero b costs
    x.copy_(torch.as_tensor(x0))
    H.cycle_async(b, x, args.warmup, use_graph=use_graph, zero_rhs=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    H.cycle_async(b, x, args.steps, use_graph=use_graph, zero_rhs=False)
    torch.cuda.synchronize()
    dt_gen = time.perf_counter() - t0
    general_rhs = {"value": round(args.steps / dt_gen, 3), "unit": "V-cycles/s",
                   "ms_per_step": round(dt_gen / args.steps * 1e3, 4),
                   "cycle_hbm_frac": round(H.cycle_bytes(stored=True) / (dt_gen / args.steps)
                                           / 1e9 / HBM_PEAK_GBPS, 4),
                   "note": "b streamed from HBM at the finest level (mlamg_hier_vcycle with a "
                           "non-NULL b); the headline passes the zero b as NULL"}
    factored = factored_p0_line(H, b, x, x0, hist, args, use_graph)

    # dominant kernel: the fine-level CSR SpMV (headline unit 1)
    A0 = H.levels[0].A
    fmt0 = A0.get_format()[0]
    xs = torch.randn(n, dtype=torch.float64, device="cuda")
    ys = torch.empty_like(xs)
    # cold launches (every operand from HBM), then back to back (x/y may stay in the MALL)
    t_spmv, t_spmv_med, t_spmv_ev = time_kernel_cold(lambda: A0.matvec(xs, out=ys), reps=20)
    t_warm = time_kernel(lambda: A0.matvec(xs, out=ys), reps=50)
    B = spmv_bytes(n, n, A0.nnz)          # SURVEY.md §8(d) CSR bytes (format independent)
    B_fmt = A0.format_bytes()             # bytes the chosen storage format actually streams
    achieved = B_fmt / t_spmv / 1e9
    # A/B of the exact-order SpMV kernels on a separate copy of A0 (same bits, different layout)
    from mlamg.sparse import DeviceCSR
    Ab = DeviceCSR.from_scipy(A, check=False)
    ab = {}
    for fmt in ("csr_stream", "sell", "sorted", "sell_dict", "rowpat"):
        Ab.set_format(fmt)
        t = time_kernel(lambda: Ab.matvec(xs, out=ys), reps=30)
        fb = Ab.format_bytes()
        ab[fmt] = {"us": round(t * 1e6, 2), "format_bytes": fb, "GBps": round(fb / t / 1e9, 1),
                   "csr_equivalent_GBps": round(B / t / 1e9, 1)}
    del Ab
    pmc = load_traffic(f"spmv_c4_pmc_{fmt0}.json")
    # only a PMC measurement of this very kernel (same format, same operator size) applies
    traffic = (pmc.get("hbm_bytes_per_launch")
               if pmc and pmc.get("algorithmic_bytes_per_launch") == B_fmt else None)
    out.update({
        "roofline": {
            "bound": "hbm",
            "kernel": f"fine-level SpMV, y = A x ({fmt0} kernel, scipy summation order)",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBPS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBPS, 4),
            "traffic": traffic,
            "algorithmic_bytes_per_launch": B_fmt,
            "csr_algorithmic_bytes_per_launch": B,
            "csr_equivalent_GBps": round(B / t_spmv / 1e9, 1),
            "avg_launch_us": round(t_spmv * 1e6, 2),
            "timing": "mean of 20 cold launches (a 512 MB read before each), each timed by the "
                      "events of its own dispatch packet (hipExtLaunchKernel)",
            "median_launch_us": round(t_spmv_med * 1e6, 2),
            "stream_event_avg_launch_us": round(t_spmv_ev * 1e6, 2),
            "warm_avg_launch_us": round(t_warm * 1e6, 2),
            "warm_frac": round(B_fmt / t_warm / 1e9 / HBM_PEAK_GBPS, 4),
        },
        # the same fine SpMV in the generic CSR-stream kernel (no stencil re-encoding: what an
        # arbitrary CSR operator gets)
        "roofline_generic_csr": {
            "kernel": "fine-level SpMV, csr_stream kernel (plain CSR, 12 B/nnz)",
            "achieved": ab["csr_stream"]["GBps"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": round(ab["csr_stream"]["GBps"] / HBM_PEAK_GBPS, 4),
            "algorithmic_bytes_per_launch": ab["csr_stream"]["format_bytes"],
            "avg_launch_us": ab["csr_stream"]["us"]},
        "fine_spmv_formats": ab,
        "conv_factor_10cycles": round(conv, 5),
        "general_rhs": general_rhs,
        "factored_p0": factored,
    })
    # host-buffer boundary: solve() on numpy b/x0 pays the PCIe copies of b
    # and x0 in and x out around its cycles; 10 cycles per call, the same hierarchy
    b_h0 = np.zeros(n)
    H.solve(b_h0, x0=x0, tol=None, maxiter=10)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        H.solve(b_h0, x0=x0, tol=None, maxiter=10)
    dt_h = (time.perf_counter() - t0) / 3
    out["pcie_inclusive"] = {
        "value": round(10 / dt_h, 3), "unit": "V-cycles/s", "cycles_per_call": 10,
        "note": "Hierarchy.solve on host numpy b, x0 (pageable; copied in, x copied out, "
                "history read back) - not the headline value"}
    if not args.no_c3:
        out["roofline_unstructured_c3"] = c3_spmv_roofline(xs.device)
    if not args.no_varcoef:
        out["variable_coefficient_c4"] = varcoef_c4(args, use_graph)
    if not args.no_cpu_baseline:
        b_h = np.zeros(n)
        v, dtc, hcpu = cpu_baseline(H, b_h, x0, args.cpu_cycles)
        # the CPU port and the device agree on the residual history (fp64 tolerance)
        agree = bool(np.allclose(hcpu[: min(3, len(hist))], hist[: min(3, len(hcpu))],
                                 rtol=1e-8))
        out["cpu_baseline"] = {
            "value": round(v, 5), "unit": "V-cycles/s", "cores": 1, "kind": "port",
            "sample": f"{args.cpu_cycles} V-cycles of the same C4 hierarchy with the scipy "
                      f"oracle (oracle/restated.py vcycle_solve), 1 thread, {dtc:.1f}s; "
                      f"host: {host_cores()[1]}; residuals agree with GPU: {agree}",
        }
        # a parallel CPU implementation of the same cycle on the box's host share (context for
        # the 1-thread port above, which is the reference's own execution model)
        thr, cores_desc = host_cores()
        vp, dtp, hp = cpu_baseline_parallel(H, b_h, x0, args.cpu_par_cycles, thr)
        agree_p = bool(np.allclose(hp[: min(3, len(hist))], hist[: min(3, len(hp))], rtol=1e-8))
        out["cpu_baseline_parallel"] = {
            "value": round(vp, 4), "unit": "V-cycles/s", "cores": thr, "kind": "port",
            "sample": f"{args.cpu_par_cycles} V-cycles of the same C4 hierarchy, OpenMP row-"
                      f"parallel CSR kernels (oracle/omp_cycle.c), {thr} threads = every CPU "
                      f"this process may use ({cores_desc}), {dtp:.1f}s; "
                      f"residuals agree with GPU: {agree_p}",
        }


def factored_p0_line(H, b, x, x0, hist, args, use_graph):
    """Opt-in factored level-0 prolongation (Hierarchy.set_factored_prolong: x += t - (w/a_ii)
    A t, t = Agg e; NOT bitwise the explicit P, tolerance-tested): its cycle rate beside the
    headline, which keeps the explicit P. Reported with its 10-cycle history's largest
    relative deviation from the explicit-P history."""
    from mlamg._lib import MlamgError
    try:
        H.set_factored_prolong(0)
    except MlamgError as e:
        return {"unsupported": str(e)}
    try:
        x.copy_(torch.as_tensor(x0))
        hf = H.cycle(b, x, 10, use_graph=use_graph)
        dev = float(np.max(np.abs(hf - hist) / hist)) if len(hf) == len(hist) else float("inf")
        x.copy_(torch.as_tensor(x0))
        H.cycle_async(b, x, args.warmup, use_graph=use_graph)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        H.cycle_async(b, x, args.steps, use_graph=use_graph)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        cyc = H.cycle_bytes(stored=True)
    finally:
        H.set_factored_prolong(0, on=False)
    return {"value": round(args.steps / dt, 3), "unit": "V-cycles/s",
            "ms_per_step": round(dt / args.steps * 1e3, 4),
            "cycle_hbm_frac": round(cyc / (dt / args.steps) / 1e9 / HBM_PEAK_GBPS, 4),
            "history_max_rel_dev_vs_explicit_P": dev,
            "note": "opt-in, not the headline: P_0 e applied as t - (w/a_ii) A_0 t (t = Agg e) "
                    "in the row-pair stencil kernel; not bitwise the explicit P"}


def varcoef_c4(args, use_graph):
    """The same V(1,1) cycle on a 216^3 7-point operator with an independent random coefficient
    on every cell face (problems.random_coeff_3d_7pt: C4's sparsity, values all distinct — no
    row-pair pattern or dictionary encoding applies, so every level streams plain 12 B/nonzero
    CSR-family formats). Reported beside the headline: its cycle rate, and its fine SpMV against
    the HBM roofline in the format the autotune chose."""
    from mlamg import problems
    from mlamg.hierarchy import Hierarchy
    t0 = time.perf_counter()
    A = problems.random_coeff_3d_7pt(args.n, seed=0)
    t_mat = time.perf_counter() - t0
    H = Hierarchy.build(A, alpha=args.alpha, strength_mode="invabs", max_coarse=args.max_coarse,
                        aggregation=args.aggregation, coarse_order=args.coarse_order)
    n = A.shape[0]
    x0 = np.random.RandomState(0).randn(n)
    x0 /= np.linalg.norm(x0)
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    x = torch.as_tensor(x0).cuda()
    hist = H.cycle(b, x, 10, use_graph=use_graph)
    conv = float((hist[-1] / hist[-4]) ** (1.0 / 3.0))
    steps = max(10, args.steps)
    H.cycle_async(b, x, args.warmup, use_graph=use_graph)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    H.cycle_async(b, x, steps, use_graph=use_graph)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    A0 = H.levels[0].A
    xs = torch.randn(n, dtype=torch.float64, device="cuda")
    ys = torch.empty_like(xs)
    t_spmv = time_kernel(lambda: A0.matvec(xs, out=ys), reps=30)
    fb = A0.format_bytes()
    cyc_fmt = H.cycle_bytes(stored=True)
    res = {
        "workload": f"3D 7-point diffusion {args.n}^3 ({n} DoF, nnz {A.nnz}), random face "
                    f"coefficients 10^U(-1,1) (all values distinct), same SA-AMG V(1,1) recipe "
                    f"({aggregation_rule(args)}), {H.n_levels} levels",
        "value": round(steps / dt, 3), "unit": "V-cycles/s", "ms_per_step": round(dt / steps * 1e3, 4),
        "conv_factor_10cycles": round(conv, 5),
        "fine_spmv": {"format": "/".join(map(str, A0.get_format()[:2])),
                      "achieved": round(fb / t_spmv / 1e9, 1), "peak": HBM_PEAK_GBPS,
                      "unit": "GB/s", "frac": round(fb / t_spmv / 1e9 / HBM_PEAK_GBPS, 4),
                      "algorithmic_bytes_per_launch": fb, "avg_launch_us": round(t_spmv * 1e6, 2)},
        "cycle_format_bytes": cyc_fmt,
        "cycle_hbm_frac": round(cyc_fmt / (dt / steps) / 1e9 / HBM_PEAK_GBPS, 4),
        "operator_formats": [{k: v[0] + (f"/{v[1]}" if v[1] else "") for k, v in f.items()}
                             for f in H.formats()],
        "setup_s": round(H.timings["total"], 3), "matrix_build_s": round(t_mat, 2),
    }
    log(f"variable-coefficient C4: {res['value']} V-cycles/s, fine SpMV "
        f"{res['fine_spmv']['format']} {res['fine_spmv']['frac']}")
    del H
    return res


def c3_spmv_roofline(device):
    """Fine SpMV of the unstructured C3 operator (P1 Laplacian on cylflow-highres refined x4^3,
    817,024 DoF; no stencil structure, so no row-pair patterns): every exact-order format
    timed, the fastest reported against the HBM peak, plus plain CSR-stream."""
    from mlamg import mesh
    from mlamg._lib import MlamgError
    from mlamg.sparse import DeviceCSR
    m = mesh.load_npz(os.path.join(ROOT, "tests", "golden", "cylflow_highres_mesh.npz"))
    A3 = mesh.poisson_dirichlet(mesh.refine(mesh.refine(mesh.refine(m))))[0]
    Ad = DeviceCSR.from_scipy(A3, check=False)
    x3 = torch.randn(A3.shape[0], dtype=torch.float64, device=device)
    y3 = torch.empty_like(x3)
    res = {}
    for fmt in ("csr_stream", "sell", "sorted", "sell_dict", "rowpat"):
        try:
            Ad.set_format(fmt)
        except MlamgError:
            continue
        t = time_kernel(lambda: Ad.matvec(x3, out=y3), reps=50)
        fb = Ad.format_bytes()
        res[fmt] = {"us": round(t * 1e6, 2), "format_bytes": fb, "GBps": round(fb / t / 1e9, 1),
                    "frac": round(fb / t / 1e9 / HBM_PEAK_GBPS, 4)}
    best = min(res, key=lambda k: res[k]["us"])
    return {"kernel": f"C3 fine SpMV ({A3.shape[0]} rows, {A3.nnz} nnz), best exact format "
                      f"{best}", "achieved": res[best]["GBps"], "peak": HBM_PEAK_GBPS,
            "unit": "GB/s", "frac": res[best]["frac"],
            "csr_stream_frac": res["csr_stream"]["frac"], "formats": res}


EXIT_DIST_MISMATCH = 4


def refuse_mismatch(e):
    """A distributed run whose iterate differs from the single-GPU one prints no value line and
    exits non-zero (every rank: the verification result is reduced over ranks)."""
    log(f"REFUSED: {e}")
    sys.exit(EXIT_DIST_MISMATCH)


def verify_selftest(world, rank):
    """--verify-selftest (CPU, gloo): the distributed verification chain with a mismatch
    injected on rank 1 (MLAMG_INJECT_MISMATCH_RANK) — the same decision and exit path as a
    real run whose iterate is wrong; no GPU work."""
    import torch.distributed as dist
    from mlamg import distributed
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo", world_size=world, rank=rank)
    bad = os.environ.get("MLAMG_INJECT_MISMATCH_RANK") == str(rank)

    class _Paths:
        def set_overlap(self, on):
            pass

        def set_cycle_graph(self, on):
            pass

    def check():
        ok = torch.tensor([0.0 if bad else 1.0])
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        return bool(ok.item() == 1.0)

    try:
        graph_on, overlap_on = distributed.verify_paths(check, _Paths(), True, True)
    except distributed.DistributedMismatch as e:
        dist.destroy_process_group()
        refuse_mismatch(e)
    if rank == 0:
        print(json.dumps({"verify_selftest": True, "value": 1.0, "cycle_graph": graph_on,
                          "overlap": overlap_on}), flush=True)
    dist.destroy_process_group()


def run_distributed(args, world, rank, local_rank):
    from mlamg import distributed
    ph = distributed.PhaseLog(rank, world)
    try:
        out, H, x0, teardown = distributed.bench_main(args, world, rank, local_rank, METRIC,
                                                      HBM_PEAK_GBPS, phases=ph)
        if rank == 0:
            if args.full and not args.no_cpu_baseline and H is not None:
                # rank 0 only, on the same (replicated) hierarchy; the others wait in teardown
                n = x0.shape[0]
                v, dtc, hcpu = cpu_baseline(H, np.zeros(n), x0, args.cpu_cycles)
                out["cpu_baseline"] = {
                    "value": round(v, 5), "unit": "V-cycles/s", "cores": 1, "kind": "port",
                    "sample": f"{args.cpu_cycles} V-cycles of the same C4 hierarchy with the "
                              f"scipy oracle (oracle/restated.py vcycle_solve), 1 thread, "
                              f"{dtc:.1f}s, rank 0's host; host: {host_cores()[1]}"}
            print(json.dumps(out), flush=True)
        teardown()
    except distributed.DistributedMismatch as e:
        refuse_mismatch(e)
    except Exception as e:  # noqa: BLE001 — name the phase, exit non-zero, never hang
        import traceback
        traceback.print_exc()
        ph.fail(f"{type(e).__name__}: {e}")


if __name__ == "__main__":
    main()
