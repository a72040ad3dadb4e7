#!/usr/bin/env python
"""Record tests/golden/greedy_cf.npz: the reference's greedy_coarsening (ns/lib/greedy.py) on the
matrices of tests/greedy_cases.py.

    python tools/make_greedy_golden.py --reference /path/to/ml-amg

The reference is imported by path; the npz holds only (case, theta, F, C). For the random-weight
cases the script walks the same algorithm once more, recording every comparison, and refuses to
write unless every dominance compared with theta is more than 1e-9 away from it and the two
smallest dominances at every pick are more than 1e-9 apart: then neither the summation order nor
a last-ulp difference can change a decision, and F and C are facts about the matrix. (Reseed the
case in tests/greedy_cases.py if it refuses.) The integer stencils have exact sums; their ties
are the point.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GAP = 1e-9


def gaps(A, theta):
    """(F, C, smallest |dominance - theta| compared, smallest gap between the two lowest
    dominances at a pick) of the greedy splitting, in plain numpy."""
    n = A.shape[0]
    ip, ij, a = A.indptr, A.indices, np.abs(A.data)
    diag = np.abs(A.diagonal())
    dom = np.array([diag[i] / a[ip[i]:ip[i + 1]].sum() for i in range(n)])
    state = np.zeros(n, dtype=int)  # 0 U, 1 F, 2 C
    g_theta, g_pick = np.abs(dom - theta).min(), np.inf
    F = [i for i in range(n) if dom[i] >= theta]
    state[F] = 1
    C = []
    while (state == 0).any():
        U = np.flatnonzero(state == 0)
        d = np.sort(dom[U])
        if len(d) > 1:
            g_pick = min(g_pick, d[1] - d[0])
        c = U[np.argmin(dom[U])]
        state[c] = 2
        C.append(c)
        for q in range(ip[c], ip[c + 1]):
            i = ij[q]
            if state[i] != 0 or A.data[q] == 0:
                continue
            cols = ij[ip[i]:ip[i + 1]]
            keep = state[cols] != 2
            dom[i] = diag[i] / a[ip[i]:ip[i + 1]][keep].sum()
            g_theta = min(g_theta, abs(dom[i] - theta))
            if dom[i] >= theta:
                state[i] = 1
                F.append(i)
    return np.array(F, dtype=int), np.array(C, dtype=int), g_theta, g_pick


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "greedy_cf.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location(
        "ref_greedy", os.path.join(args.reference, "ns", "lib", "greedy.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    import greedy_cases as gc

    out = {}
    for name, (build, theta, exact) in gc.CASES.items():
        A = build()
        nF, F, C = ref.greedy_coarsening(A, theta)
        F, C = np.asarray(F, dtype=np.int64), np.asarray(C, dtype=np.int64)
        assert nF == len(F) and len(F) + len(C) == A.shape[0]
        F2, C2, g_theta, g_pick = gaps(A, theta)
        assert np.array_equal(F, F2) and np.array_equal(C, C2), name
        if not exact:
            assert g_theta > GAP and g_pick > GAP, (name, g_theta, g_pick, "reseed this case")
        print(f"{name}: n {A.shape[0]} theta {theta} |F| {len(F)} |C| {len(C)} "
              f"gap to theta {g_theta:.3e} gap at picks {g_pick:.3e} "
              f"C sorted {bool(np.all(np.diff(C) > 0))}")
        out[f"{name}_theta"] = np.float64(theta)
        out[f"{name}_F"] = F
        out[f"{name}_C"] = C
    out["cases"] = np.array(sorted(gc.CASES))
    np.savez(args.out, **out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
