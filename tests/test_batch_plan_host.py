"""The batched solver's host planner (csrc/batch_plan.cpp) on the CPU: compiled with plain g++
together with tests/host/batch_plan_driver.cpp and compared with a numpy restatement of its rules
(level schedule, half-bandwidth of P^T A P, exact symmetry, slot widths, LDS budgets). The planner
decides which kernel variant runs and where every array lies in the arena; here its decisions are
checked without a device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml-amg_amd", "csrc")
OK, EINVAL, EUNSUPPORTED = 0, -1, -5
LDS = 156 * 1024  # batch_plan.hpp kBLdsBytes


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("batch_plan") / "driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", f"-I{CSRC}",
                    os.path.join(CSRC, "batch_plan.cpp"),
                    os.path.join(ROOT, "tests", "host", "batch_plan_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def plan(driver, tmp_path, problems, passes=1, smoother=0, env=None):
    """problems: (n, n_c, A, P) with A, P = (indptr, indices, data) -> parsed driver records."""
    words = [passes, smoother, 1, 1, 5, len(problems)]
    for n, nc, A, P in problems:
        words += [n, nc, len(A[1]), len(P[1])]
        for M in (A, P):
            words += list(M[0]) + list(M[1]) + [repr(float(v)) for v in M[2]]
    path = tmp_path / "in.txt"
    path.write_text(" ".join(str(w) for w in words))
    e = {k: v for k, v in os.environ.items() if not k.startswith("MLAMG_")}
    e.update(env or {})
    r = subprocess.run([driver, str(path)], capture_output=True, text=True, env=e, timeout=60)
    assert r.returncode == 0, r.stderr
    out = [dict(plan=None, prob={}, lev={}, pkr0={}) for _ in range(passes)]
    cur = None
    for line in r.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        if kind == "plan":
            head, err = rest.split(" err=", 1)
            cur = out[int(re.match(r"pass=(\d+)", head).group(1))]
            cur["plan"] = dict((k, int(v)) for k, v in (f.split("=") for f in head.split()))
            cur["plan"]["err"] = err
        elif kind == "prob":
            q, fields = rest.split(" ", 1)
            cur["prob"][int(q)] = dict((k, int(v)) for k, v in (f.split("=") for f in fields.split()))
        else:
            q, vals = rest.split(":")
            cur[kind][int(q)] = [int(v) for v in vals.split()]
    return out


def csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return (M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64))


def poisson_1d(n):
    return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n), format="csr")


def poisson_2d(m):
    I = sp.identity(m)
    return sp.csr_matrix(sp.kron(I, poisson_1d(m)) + sp.kron(poisson_1d(m), I))


def aggregates(agg):
    agg = np.asarray(agg)
    return sp.csr_matrix((np.ones(len(agg)), (np.arange(len(agg)), agg)))


def grid_problem_1d(n=12, box=3):
    return (n, n // box, csr(poisson_1d(n)), csr(aggregates(np.arange(n) // box)))


def grid_problem_2d(m=6, box=3):
    i, j = np.divmod(np.arange(m * m), m)
    return (m * m, (m // box) ** 2, csr(poisson_2d(m)), csr(aggregates((i // box) * (m // box) + j // box)))


# ---------------------------------------------------------------- the rules, restated
def restate(problem, no_band=False):
    """What the planner must decide for one problem of a Gauss-Seidel, non-phased batch."""
    n, nc, (aip, aij, av), (pip, pij, pv) = problem
    rows = np.repeat(np.arange(n), np.diff(aip))
    # level(i) = 1 + max level(j) over j < i coupled in either direction; rows ascending in a level
    nbr = [set() for _ in range(n)]
    for i, j in zip(rows, aij):
        if i != j:
            nbr[i].add(j)
            nbr[j].add(i)
    level = np.zeros(n, dtype=np.int64)
    for i in range(n):
        level[i] = max([level[j] + 1 for j in nbr[i] if j < i], default=0)
    nlev = int(level.max()) + 1
    lev = np.concatenate([[0], np.cumsum(np.bincount(level, minlength=nlev))])
    pkr0 = np.argsort(level, kind="stable")
    # exact symmetry, entry by entry (values included)
    ent = sorted(zip(rows, aij, av))
    sym = ent == sorted(zip(aij, rows, av))
    # half-bandwidth of the structure of P^T A P
    As = sp.csr_matrix((np.ones(len(aij)), aij, aip), shape=(n, n))
    Ps = sp.csr_matrix((np.ones(len(pij)), pij, pip), shape=(n, nc))
    I, J = (Ps.T @ As @ Ps).nonzero()
    band = int(np.max(I - J, initial=0))
    band_w = 1
    while band_w < band + 2:
        band_w *= 2
    banded = sym and not no_band and band <= 63 and nc <= 1024 and 8 * (band_w * (band_w + 1) + band_w) <= LDS
    # slot widths
    maxoff = int(np.bincount(rows[rows != aij], minlength=n).max())
    wmax = int(np.diff(lev).max())
    KA = max(1, int(np.diff(aip).max()))
    KP = max(1, int(np.diff(pip).max()))
    KT = max(1, int(np.bincount(pij, minlength=nc).max()))
    # LDS: x and r (both fit at these sizes), r_H and e_H; the staging area gets the rest
    vec = n * 16 + 16 + nc * 16
    assert vec + 16 * 1024 <= LDS
    room = LDS - vec - 64
    km = 4 if maxoff <= 4 else 8 if maxoff <= 8 else 0
    gs_rw = (1 if wmax <= 64 else 2 if wmax <= 128 else 0) if km == 4 else int(km == 8 and wmax <= 64)
    if gs_rw and min(4096, room // (12 * km + 24)) - 1 < wmax:
        gs_rw = 0
    gs_db = int(bool(gs_rw) and min(4096, room // (2 * (12 * km + 24) + 16)) - 1 >= 3 * wmax)
    K = km if gs_rw else max(maxoff, 1)
    cap = min(4096, (room - (32 if gs_db else 0)) // ((12 * K + 24) * (2 if gs_db else 1))) - 1
    n_chunks, l = 0, 0
    while l < nlev:
        start, cnt = l, 0
        while l < nlev and (l == start or cnt + lev[l + 1] - lev[l] <= cap):
            cnt += lev[l + 1] - lev[l]
            l += 1
        n_chunks += 1
    chol = lambda nb: 8 * (2 * nb * (nb + 1) + nc * (nb + 1) + nb * nc)
    chol_nb = next(nb for nb in (16, 8, 4) if chol(nb) <= LDS or nb == 4)
    panel = next(b for b in (16, 8, 4) if nc * (b + 1) * 8 + 16 * b + nc * 12 <= LDS or b == 4)
    rec = dict(spd=int(sym and not banded and chol(chol_nb) <= LDS), band_ld=band + 1 if banded else 0,
               nlev=nlev, K=K, KA=KA, KP=KP, KT=KT, panel=panel, chol_nb=chol_nb, gs_rw=gs_rw,
               gs_db=gs_db, gs_rp=0, n_chunks=n_chunks, cap=cap, setup_mode=0, phased=0)
    return rec, list(lev), list(pkr0)


STRUCT = ("spd band_ld nlev K KA KP KT panel chol_nb gs_rw gs_db gs_rp n_chunks cap setup_mode "
          "phased").split()


def check(result, problems, **kw):
    assert result["plan"]["code"] == OK, result["plan"]
    for q, problem in enumerate(problems):
        rec, lev, pkr0 = restate(problem, **kw)
        got = result["prob"][q]
        assert {k: got[k] for k in STRUCT} == rec, q
        assert result["lev"][q] == lev and result["pkr0"][q] == pkr0, q


# ---------------------------------------------------------------- cases
def test_poisson_1d_band(driver, tmp_path):
    prob = grid_problem_1d()
    (res,) = plan(driver, tmp_path, [prob])
    check(res, [prob])
    got = res["prob"][0]
    assert prob[1] == 4 and got["nlev"] == 12 and res["lev"][0] == list(range(13))
    assert got["band_ld"] == 2 and got["spd"] == 0 and res["plan"]["any_band"] == 1


def test_poisson_2d_antidiagonal_levels(driver, tmp_path):
    prob = grid_problem_2d()
    (res,) = plan(driver, tmp_path, [prob])
    check(res, [prob])
    got = res["prob"][0]
    assert got["gs_rw"] == 1 and got["K"] == 4 and got["nlev"] == 11
    i, j = np.divmod(np.array(res["pkr0"][0]), 6)
    assert list(np.repeat(np.arange(11), np.diff(res["lev"][0]))) == list(i + j)


def test_unsymmetric_value_drops_the_band(driver, tmp_path):
    prob = grid_problem_2d()
    sym = plan(driver, tmp_path, [prob])[0]["prob"][0]
    aip, aij, av = prob[2]
    av = av.copy()
    av[aip[7]] *= 1.0 + 2.0 ** -52  # one off-diagonal entry, its mirror untouched
    assert aij[aip[7]] != 7
    unsym = (prob[0], prob[1], (aip, aij, av), prob[3])
    (res,) = plan(driver, tmp_path, [unsym])
    check(res, [unsym])
    got = res["prob"][0]
    assert got["spd"] == 0 and got["band_ld"] == 0 and sym["band_ld"] > 0
    skip = ("spd", "band_ld")
    assert {k: got[k] for k in STRUCT if k not in skip} == {k: sym[k] for k in STRUCT if k not in skip}


@pytest.mark.parametrize("mirrored", [True, False])
def test_repeated_column(driver, tmp_path, mirrored):
    """Rows 0 and 1 store their coupling twice (-0.5, -0.5): symmetric entry by entry when both
    do; when row 1 stores it once (-1.0) only the summed matrix is symmetric, which does not
    count."""
    n = 12
    aip, aij, av = (list(x) for x in csr(poisson_1d(n)))
    # row 0 = (0: 2, 1: -1) -> (0: 2, 1: -0.5, 1: -0.5)
    aij[1:2], av[1:2] = [1, 1], [-0.5, -0.5]
    aip = [aip[0]] + [p + 1 for p in aip[1:]]
    if mirrored:  # row 1 = (0: -1, 1: 2, 2: -1) -> (0: -0.5, 0: -0.5, 1: 2, 2: -1)
        k = aip[1]
        aij[k:k + 1], av[k:k + 1] = [0, 0], [-0.5, -0.5]
        aip = aip[:2] + [p + 1 for p in aip[2:]]
    prob = (n, 4, (np.array(aip), np.array(aij), np.array(av)), grid_problem_1d()[3])
    (res,) = plan(driver, tmp_path, [prob])
    check(res, [prob])
    assert (res["prob"][0]["band_ld"] > 0) == mirrored


def test_rows_too_long(driver, tmp_path):
    n = 40
    Pm = csr(aggregates(np.arange(n) // 4))
    A = sp.lil_matrix(poisson_1d(n))
    A[0, 1:35] = -1.0  # 34 off-diagonals and the diagonal: 35 slots
    (res,) = plan(driver, tmp_path, [(n, 10, csr(A), Pm)])
    assert res["plan"]["code"] == EUNSUPPORTED and res["plan"]["err"] == (
        "amg2v_batch: rows of A, P or P^T longer than the batched solver's slots (problem 0)")
    A = sp.lil_matrix(poisson_1d(n))
    A[0, 0] = 0.0
    A[0, 1:34] = -1.0  # 33 slots hold the row, but the sweep has 32 off-diagonal slots
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    (res,) = plan(driver, tmp_path, [grid_problem_1d(), (n, 10, csr(A), Pm)])
    assert res["plan"]["code"] == EUNSUPPORTED and res["plan"]["err"] == (
        "amg2v_batch: a row of A has more than 32 off-diagonal entries (problem 1)")
    n = 258  # 257 fine rows in one aggregate: a row of P^T with 257 entries
    Pm = csr(aggregates([0] * 257 + [1]))
    (res,) = plan(driver, tmp_path, [(n, 2, csr(poisson_1d(n)), Pm)])
    assert res["plan"]["code"] == EUNSUPPORTED and res["plan"]["err"] == (
        "amg2v_batch: rows of A, P or P^T longer than the batched solver's slots (problem 0)")


def test_invalid_input_names_the_problem(driver, tmp_path):
    good = grid_problem_1d()
    n, nc, (aip, aij, av), Pm = good
    (res,) = plan(driver, tmp_path, [good, (n, n + 1, (aip, aij, av), Pm)])
    assert (res["plan"]["code"], res["plan"]["err"]) == (EINVAL, "coarse size out of range (problem 1)")
    bad = aip.copy()
    bad[3], bad[4] = aip[4], aip[3]  # descending
    (res,) = plan(driver, tmp_path, [good, good, (n, nc, (bad, aij, av), Pm)])
    assert (res["plan"]["code"], res["plan"]["err"]) == (EINVAL, "A is not a valid n x n CSR (problem 2)")
    bad = aij.copy()
    bad[5] = n
    (res,) = plan(driver, tmp_path, [(n, nc, (aip, bad, av), Pm), good])
    assert (res["plan"]["code"], res["plan"]["err"]) == (EINVAL, "A is not a valid n x n CSR (problem 0)")
    bad = Pm[1].copy()
    bad[0] = nc
    (res,) = plan(driver, tmp_path, [good, (n, nc, (aip, aij, av), (Pm[0], bad, Pm[2]))])
    assert (res["plan"]["code"], res["plan"]["err"]) == (EINVAL, "P is not a valid n x n_c CSR (problem 1)")


def test_shared_pattern_shares_the_structure(driver, tmp_path):
    a, b = grid_problem_2d(), grid_problem_1d()
    c = (a[0], a[1], (a[2][0], a[2][1], 3.0 * a[2][2]), a[3])  # a's pattern, other values
    (res,) = plan(driver, tmp_path, [a, b, c])
    check(res, [a, b, c])
    pa, pb, pc = (res["prob"][q] for q in range(3))
    assert {k: pa[k] for k in STRUCT} == {k: pc[k] for k in STRUCT}
    assert (pa["ak_col"], pa["pk_row0"]) == (pc["ak_col"], pc["pk_row0"])
    assert pa["ak_col"] != pb["ak_col"] and pa["pk_row0"] != pb["pk_row0"]
    assert len({pa["a_raw"], pb["a_raw"], pc["a_raw"]}) == 3 and len({pa["b"], pb["b"], pc["b"]}) == 3


def test_host_threads_and_caches(driver, tmp_path):
    """Eight problems on four host threads (the worker pool really hands out work), planned twice:
    the second pass is served from the pattern and shape caches and must decide the same."""
    probs = [grid_problem_2d(), grid_problem_1d(), grid_problem_1d(15, 3), grid_problem_2d(9, 3)] * 2
    first, second = plan(driver, tmp_path, probs, passes=2, env={"MLAMG_HOST_THREADS": "4"})
    check(first, probs)
    assert first["prob"] == second["prob"] and first["lev"] == second["lev"]
    assert first["pkr0"] == second["pkr0"]
    assert {k: v for k, v in first["plan"].items() if k != "pass"} == \
           {k: v for k, v in second["plan"].items() if k != "pass"}
    (inline,) = plan(driver, tmp_path, probs, env={"MLAMG_HOST_THREADS": "1"})
    assert inline["prob"] == first["prob"] and inline["pkr0"] == first["pkr0"]


def test_single_large_dense_coarse_runs_phased(driver, tmp_path):
    """One problem, symmetric, n_c = 301 > 300 and the band switched off: the device-wide coarse
    factor (setup_mode 1) and phased cycles; unsymmetric: phased with the setup kernel's factor."""
    n = 301
    prob = (n, n, csr(poisson_1d(n)), csr(aggregates(np.arange(n))))
    (res,) = plan(driver, tmp_path, [prob], env={"MLAMG_BATCH_NO_BAND": "1"})
    got = res["prob"][0]
    assert res["plan"]["code"] == OK and res["plan"]["phased"] == 1 and res["plan"]["ext_coarse"] == 1
    assert (got["spd"], got["band_ld"], got["setup_mode"], got["phased"]) == (1, 0, 1, 1)
    assert res["plan"]["two_pass"] == 0
    (res,) = plan(driver, tmp_path, [prob])  # the band is taken: nothing dense, one launch
    assert res["plan"]["phased"] == 0 and res["prob"][0]["band_ld"] == 2
    (res,) = plan(driver, tmp_path, [prob], env={"MLAMG_BATCH_NO_BAND": "1", "MLAMG_BATCH_NO_EXT": "1"})
    assert res["plan"]["phased"] == 0 and res["prob"][0]["setup_mode"] == 0
