"""Population-stacked FullAggNet fitness against the loop over the individuals, on
the device.

The genetic algorithm of utils/train_dataset.py scores a population of weight vectors (default 20)
on a batch of small grids every generation. Dataset and networks are those of
tools/bench_gnn_batch.py: nb in {16, 64} grids of 16^2 .. 48^2 nodes, FullAggNet(8, num_conv=2,
iterations=2) (the network that is trained) and the default FullAggNet() (dim 64), seeded
weights with positive biases; the population is the net's own vector plus seeded perturbations in
+-0.02. For each combination, in this one process:

  fitness   fitness.population_fitness_stacked   vs  fitness.population_fitness (the loop of
            evaluate_dataset, one load_state_dict and one forward_stack per individual)
  forward   FullAggNet.forward_population        vs  the loop load_state_dict -> forward_stack

The two sides alternate, `rounds` times `reps` repetitions each, after a warm-up pass of the same
shapes (which also builds the cached PopulationBatch and its Bellman-Ford plan: a generation
after the first does not pay for them; their one-off cost is recorded as setup_ms). Every figure
is a host clock around work that ends in a device synchronise or a download: mean, standard
deviation and minimum over all repetitions and the mean of every round, in ms. The ratio is loop
mean / stacked mean; below 1 the stacked path lost. Before anything is timed the stacked
convergence factors are compared with the loop's, bitwise.

GPU box: python tools/bench_gnn_population.py [--out profiles/gnn/population.json] [--nb 16 64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-amg_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_gnn_batch import ALPHA, dataset, network  # noqa: E402
from mlamg import fitness, gnn, multigrid  # noqa: E402

POPULATION = 20  # train_dataset.py's default


def population(net, members):
    w0 = fitness.weights_as_vector(net)
    rs = np.random.RandomState(members)
    return np.stack([w0] + [w0 + rs.uniform(-0.02, 0.02, w0.size).astype(np.float32)
                            for _ in range(members - 1)])


def once(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(stacked, loop, rounds, reps):
    stacked(), loop()  # warm-up: the same shapes as the timed passes
    torch.cuda.synchronize()
    ts = {"stacked": [], "loop": []}
    for _ in range(rounds):
        for name, fn in (("stacked", stacked), ("loop", loop)):
            ts[name].append([once(fn) for _ in range(reps)])
    out = {}
    for name, rows in ts.items():
        a = np.array(rows)
        out[name] = {"mean_ms": round(float(a.mean()), 3), "std_ms": round(float(a.std()), 3),
                     "min_ms": round(float(a.min()), 3),
                     "round_means_ms": [round(float(r.mean()), 3) for r in a],
                     "reps": int(a.size)}
    out["ratio"] = round(out["loop"]["mean_ms"] / out["stacked"]["mean_ms"], 2)
    return out


def run(net, As, members, rounds, reps):
    batch = gnn.GraphBatch(As)
    pop = population(net, members)
    own = fitness.weights_as_dict(net, pop[0])
    per = min(net.members_per_pass(batch), members)
    passes = [min(per, members - a) for a in range(0, members, per)]
    row = {"nb": len(As), "nodes": int(batch.n), "edges": int(batch.E), "population": members,
           "members_per_pass": int(per), "passes": len(passes)}
    row["setup_ms"] = round(once(lambda: [batch.population(m).plan() for m in set(passes)]), 3)
    # solve_batches: 1 = one amg_2_v_batch over every (member, grid) problem; 1 + members = the
    # fused solver refused the joint batch and the solves were cut by member, as in the loop
    calls, real = [], multigrid.amg_2_v_batch

    def counted(problems, **kw):
        calls.append("engine" not in kw)  # its own call for the per-problem path has it
        return real(problems, **kw)

    multigrid.amg_2_v_batch = counted
    try:
        conv = fitness.evaluate_population(net, pop, batch, ALPHA)
    finally:
        multigrid.amg_2_v_batch = real
    row["solve_batches"] = int(sum(calls))
    ref = np.stack([fitness.evaluate_dataset(net, batch, ALPHA, weights=w) for w in pop])
    assert np.array_equal(conv, ref), "stacked and looped convergence factors differ"
    row["failed_problems"] = int((ref == 1.0).sum())
    row["mean_conv"] = round(float(ref.mean()), 6)

    def loop_forward():
        for w in pop:
            net.load_state_dict(fitness.weights_as_dict(net, w))
            net.forward_stack(batch, ALPHA)

    row["fitness"] = alternate(lambda: fitness.population_fitness_stacked(net, pop, batch, ALPHA),
                               lambda: fitness.population_fitness(net, pop, batch, ALPHA),
                               rounds, reps)
    row["forward"] = alternate(lambda: net.forward_population(batch, pop, ALPHA), loop_forward,
                               rounds, reps)
    net.load_state_dict(own)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn", "population.json"))
    ap.add_argument("--nb", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--population", type=int, default=POPULATION)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    nets = {"dim8_conv2_it2": network(8, num_conv=2, iterations=2), "dim64_default": network(64)}
    out = {"device": torch.cuda.get_device_name(0), "alpha": ALPHA,
           "grids": "16^2..48^2, Poisson / jump coefficient alternating",
           "timing": "host clock to a device synchronise; stacked and loop alternate, "
                     f"{args.rounds} rounds x {args.reps} repetitions after a warm-up of both",
           "results": []}
    for name, net in nets.items():
        for nb in args.nb:
            row = {"network": name, **run(net, dataset(nb), args.population, args.rounds,
                                          args.reps)}
            print(json.dumps(row), flush=True)
            out["results"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
