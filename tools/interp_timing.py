"""Timing of the learned-P setup on the device.

For Poisson grids of 32^2, 64^2 and 128^2 nodes (greedy C/F splitting at theta 0.56, seeded
weights), in this one process:

  forward_mat    InterpolationNetwork.forward_mat(A, C, F), host graph construction included
  network        ResidualBlock.run on the prebuilt graph (nodes / edges: its two halves)
  baseline       the plain-torch float32 restatement (tests/interp_ref.py: matmul / index_add_,
                 hipBLASLt underneath) of the same network on the same GPU and the same graph
  greedy         mlamg.greedy.greedy_coarsening on the host

and mlamg_gnn_linear_wide alone at (M, 256, 256) against torch.matmul, with the achieved TFLOP/s
(2 M K N operations over the median time).

Every figure is a host clock around work that ends in a device synchronise, after warm-up passes
of the same shapes: median, minimum and maximum over the repetitions, in ms. The device's edge
values are compared with the baseline's before anything is timed.

GPU box: python tools/interp_timing.py [--out profiles/gnn/interp.json] [--grids 32 64 128]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-amg_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import interp_ref  # noqa: E402
from mlamg import interp, problems  # noqa: E402
from mlamg.greedy import greedy_coarsening  # noqa: E402


def timed(fn, reps, warm=2, sync=True):
    for _ in range(warm):
        fn()
    if sync:
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3),
            "max_ms": round(float(ts.max()), 3), "reps": reps}


def grid_row(net, sd, m, reps):
    A = problems.poisson_2d_5pt(m)
    _, F, C = greedy_coarsening(A, 0.56)
    g = net.graph_from_matrix(A, C, F)
    model = net.model
    ref = interp_ref.Ref(sd, g.src.cpu().numpy(), g.tgt.cpu().numpy(),
                         g.edge_attr.cpu().numpy()[:, 0], torch.float32, device="cuda")
    with torch.no_grad():
        dev = model.run(g)
        base = ref.forward(g.x)[1]
        x = model.run_nodes(g)
    scale = float(base.abs().max())
    row = {"grid": m, "nodes": int(g.n), "coarse": int(len(C)), "edges": int(g.E),
           "max_abs_diff_to_baseline_over_scale": float((dev - base).abs().max()) / scale}
    with torch.no_grad():
        row["greedy_host"] = timed(lambda: greedy_coarsening(A, 0.56), max(3, reps // 3), 1, False)
        row["forward_mat"] = timed(lambda: net.forward_mat(A, C, F), reps)
        row["network"] = timed(lambda: model.run(g), reps)
        row["network_nodes"] = timed(lambda: model.run_nodes(g), reps)
        row["network_edges"] = timed(lambda: interp.standardize_abs(model.edge_model.run(g, x)),
                                     reps)
        row["baseline"] = timed(lambda: ref.forward(g.x), reps)

        def base_nodes():
            y = ref.t(g.x)
            for i in range(len(interp_ref.NODE_BLOCKS)):
                y = ref.node_layer(i, y)
            return y

        def base_edges():
            e = x
            for i in range(interp_ref.N_EDGE_BLOCKS):
                e = ref.edge_layer(i, e)
            return ref.standardize(e)

        row["baseline_nodes"] = timed(base_nodes, reps)
        row["baseline_edges"] = timed(base_edges, reps)
    for k in ("network", "network_nodes", "network_edges"):
        b = row[k.replace("network", "baseline")]["median_ms"]
        row[k]["baseline_over_device"] = round(b / row[k]["median_ms"], 3)
    return row


def linear_row(M, reps):
    gen = torch.Generator().manual_seed(M)
    X = torch.randn(M, 256, generator=gen).cuda()
    W = (torch.randn(256, 256, generator=gen) / 16).cuda()
    Y = torch.empty(M, 256, device="cuda")
    got, want = interp.linear_wide(X, W), X @ W.T
    row = {"M": M, "K": 256, "N": 256,
           "max_abs_diff_over_scale": float((got - want).abs().max() / want.abs().max()),
           "linear_wide": timed(lambda: interp.linear_wide(X, W, out=Y), reps, warm=3),
           "torch_matmul": timed(lambda: torch.matmul(X, W.T, out=Y), reps, warm=3)}
    for k in ("linear_wide", "torch_matmul"):
        row[k]["tflops"] = round(2.0 * M * 256 * 256 / (row[k]["median_ms"] * 1e-3) / 1e12, 3)
    row["matmul_over_wide"] = round(row["torch_matmul"]["median_ms"]
                                    / row["linear_wide"]["median_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn", "interp.json"))
    ap.add_argument("--grids", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    net = interp.InterpolationNetwork()
    sd = {k: v.clone() for k, v in interp_ref.seeded_state_dict(net.model, 2024).items()}
    net.cuda().eval()
    out = {"device": torch.cuda.get_device_name(0), "theta": 0.56, "grids": [], "linear": []}
    for m in args.grids:
        row = grid_row(net, sd, m, args.reps)
        print(json.dumps(row), flush=True)
        out["grids"].append(row)
    for M in (4096, 16384, 65536, 262144):
        row = linear_row(M, 4 * args.reps)
        print(json.dumps(row), flush=True)
        out["linear"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
