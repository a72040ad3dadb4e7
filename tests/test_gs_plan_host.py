"""The Gauss-Seidel host planner (csrc/gs_plan.cpp) on the CPU: compiled with g++ together with
tests/host/gs_plan_driver.cpp, once plainly and once with the address and undefined-behaviour
sanitizers, and checked three ways: against a numpy restatement of its rules on small matrices,
against invariants that do not depend on that restatement (on the GPU tests' own matrices at their
real sizes too), and against the table of which matrix takes which kernel. The plan decides every
LDS ring size, slot code and step the sweep kernels trust; here it is checked without a device."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import gs_cases as gc
from gs_cases import LEVELS, PIPE, PIPE_LDS, RING, WAVE, WINDOW, WORKGROUP, WRING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml-amg_amd", "csrc")
KNOBS = ("NO_WIN", "NO_RING", "NO_LDS", "NO_WRING", "NO_WAVE")
BLOCK, BLOCK_MAX_LEVEL_ROWS, LDS_MAX, RING_MAX_LOG2 = 1024, 8192, 8192, 13  # gs_plan.hpp
BUDGET = 150 * 1024  # ring, long-row ring and window alike
RING_PAD, RING_LATER = 0xFFFF, 0xFFFE
WRING_PAD, WRING_LATER, WRING_DIAG, WRING_FAR = -1, -2, -3, -16


@pytest.fixture(scope="module", params=("plain", "sanitized"))
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("gs_plan") / f"driver_{request.param}")
    flags = ["-O1"]
    if request.param == "sanitized":
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([cxx, "-std=c++17", *flags, f"-I{CSRC}", os.path.join(CSRC, "gs_plan.cpp"),
                        os.path.join(ROOT, "tests", "host", "gs_plan_driver.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and request.param == "sanitized" and any(
            w in r.stderr for w in ("-lasan", "-lubsan", "libasan", "libubsan")):
        pytest.skip("the sanitizer runtime is not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    return exe


def plan(driver, tmp_path, A, backward=False, knobs=(), block=False, wave_lpr=0):
    """A: scipy CSR, stored order kept -> (scalars dict, arrays dict) of the driver."""
    assert set(knobs) <= set(KNOBS)
    head = [A.shape[0], A.nnz, int(backward), int(block)] + [int(k in knobs) for k in KNOBS]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.asarray(head + [wave_lpr], dtype=np.int32).tofile(f)
        A.indptr.astype(np.int32).tofile(f)
        A.indices.astype(np.int32).tofile(f)
        A.data.astype(np.float64).tofile(f)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MLAMG_")}
    r = subprocess.run([driver, str(fin), str(fout)], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0].startswith("scalars ")
    S = {k: int(v) for k, v in (f.split("=") for f in lines[0].split()[1:])}
    raw, at, arrays = fout.read_bytes(), 0, {}
    for line in lines[1:]:
        _, name, dtype, count = line.split()
        dt = np.dtype({"i4": np.int32, "u2": np.uint16, "f8": np.float64}[dtype])
        arrays[name] = np.frombuffer(raw, dtype=dt, count=int(count), offset=at).astype(
            np.int64 if dtype != "f8" else np.float64)
        at += int(count) * dt.itemsize
    assert at == len(raw)
    return S, arrays


# ---------------------------------------------------------------- the rules, restated
def ceil_log2(v):
    lg = 0
    while (1 << lg) < v:
        lg += 1
    return lg


def a16(b):
    return (b + 15) // 16 * 16


def win_buf_bytes(cap, K):
    """One staging buffer: 16-byte header, then 16-byte aligned values, diagonal, b, level starts
    (cap + 2 int32) and uint16 columns of cap + 1 positions."""
    return (16 + a16(8 * (cap + 1) * K) + 2 * a16(8 * (cap + 1)) + a16(4 * (cap + 2))
            + a16(2 * (cap + 1) * K))


def widest_span(lp, w):
    return max((lp[l + 1] - lp[max(0, l - w)] for l in range(len(lp) - 1)), default=0)


def restate(A, backward=False, knobs=(), wave_lpr=0):
    """What the planner must decide, from the rules of the sweep's documentation: plain Python
    over the rows (small matrices only)."""
    n = A.shape[0]
    ip, ij = A.indptr, A.indices
    R = {}
    nbr = [set() for _ in range(n)]
    for i in range(n):
        for j in ij[ip[i]:ip[i + 1]]:
            if i != j:
                nbr[i].add(int(j))
                nbr[j].add(i)
    level = np.zeros(n, dtype=np.int64)
    for i in (range(n - 1, -1, -1) if backward else range(n)):
        level[i] = max([level[j] + 1 for j in nbr[i] if (j > i if backward else j < i)], default=0)
    nlev = int(level.max()) + 1 if n else 0
    lp = np.concatenate([[0], np.cumsum(np.bincount(level, minlength=nlev))]).astype(np.int64)
    rows = np.argsort(level, kind="stable")
    pos = np.empty(n, dtype=np.int64)
    pos[rows] = np.arange(n)
    offd = [[int(j) for j in ij[ip[i]:ip[i + 1]] if j != i] for i in range(n)]
    max_off = max((len(o) for o in offd), default=0)
    max_len = int(np.diff(ip).max()) if n else 0
    mlr = int(np.diff(lp).max()) if nlev else 0
    K = 4 if max_off <= 4 else 8 if max_off <= 8 else 0
    deep = nlev > 4
    reach = [level[i] - level[j] for i in range(n) for j in offd[i]]
    W_earlier, W_both = max(reach + [0]), max([abs(d) for d in reach] + [0])
    R.update(level=level, level_ptr=lp, rows=rows, n_levels=nlev, max_level_rows=mlr,
             max_off=max_off, max_len=max_len, K=K, path=None)
    packed = K != 0 and mlr <= 2 * BLOCK
    if packed:
        pcol = np.full((n, K), -1, dtype=np.int64)
        for p, i in enumerate(rows):
            pcol[p, :len(offd[i])] = offd[i]
        R["pcol"] = pcol.ravel()
        rw = -(-mlr // 64)
        if "NO_WIN" not in knobs and 1 <= rw <= 8 and deep:
            cap = 4096
            while cap >= mlr and R["path"] is None:
                clev, l = [0], 0
                while l < nlev:
                    start = l
                    while l < nlev and (l == start or lp[l + 1] - lp[start] <= cap):
                        l += 1
                    clev.append(l)
                nch = len(clev) - 1
                span = max(lp[min(nlev, clev[min(ch + 2, nch)] + W_both)] - lp[max(0, clev[ch] - W_both)]
                           for ch in range(nch))
                lg = ceil_log2(span)
                if ((1 << lg) + 4) * 8 + 2 * win_buf_bytes(cap, K) <= BUDGET:
                    recs, starts = [], []
                    for ch in range(nch):
                        l0, l1 = clev[ch], clev[ch + 1]
                        la = 0 if ch == 0 else min(nlev, l0 + W_both)
                        lb = min(nlev, l1 + W_both)
                        recs += [l1 - l0, lp[l0], lp[l1] - lp[l0], lp[la], lp[lb] - lp[la],
                                 len(starts), 0, 0]
                        starts += [lp[l] - lp[l0] for l in range(l0, l1 + 1)]
                    R.update(path=WINDOW, win_w=W_both, win_cap=cap, ring_log2=lg, n_chunks=nch,
                             win_rw=rw, clev=np.array(recs + starts, dtype=np.int64),
                             wcol=np.where(pcol >= 0, pos[np.maximum(pcol, 0)], -1).ravel())
                cap = cap * 7 // 8
        if R["path"] is None and "NO_RING" not in knobs and K == 4 and mlr <= BLOCK and deep:
            lg = ceil_log2(widest_span(lp, W_earlier))
            if lg <= RING_MAX_LOG2 and 8 * (1 << lg) + 8 + 4 * (nlev + 1) <= BUDGET:
                earlier = (pcol >= 0) & (level[np.maximum(pcol, 0)] < level[rows][:, None])
                code = np.where(pcol < 0, RING_PAD,
                                np.where(earlier, pos[np.maximum(pcol, 0)] & ((1 << lg) - 1),
                                         RING_LATER))
                R.update(path=RING, ring_w=W_earlier, ring_log2_r=lg, rcode=code.ravel())
        if R["path"] is None and deep:
            lds = "NO_LDS" not in knobs and mlr <= BLOCK and n <= LDS_MAX
            R["path"] = PIPE_LDS if lds else PIPE
    elif K == 0 and max_len <= 128 and mlr <= BLOCK_MAX_LEVEL_ROWS:
        wide = n > 64 * nlev
        if "NO_WRING" not in knobs and n and deep and max_len <= 64:
            lpr = 8 if wide and max_len <= 32 else 16
            epl = 2 if max_len <= 2 * lpr else 4
            rps = (1024 if epl == 2 else 512) // lpr
            st = [(a, min(rps, lp[l + 1] - a)) for l in range(nlev) for a in range(lp[l], lp[l + 1], rps)]
            rest = 24 + 10 * rps * lpr * epl + 8 + 8 * len(st) + 16
            if max_len <= lpr * epl and len(st) <= 2 * nlev and rest < BUDGET:
                cap = 8192
                while cap > 1 and rest + 8 * cap > BUDGET:
                    cap //= 2
                Wr = W_earlier
                while Wr > 2 and widest_span(lp, Wr) > cap:
                    Wr = max(2, Wr * 7 // 8)
                lg = ceil_log2(widest_span(lp, Wr))
                if widest_span(lp, Wr) <= cap and not (Wr < W_earlier and Wr < 2) and (1 << lg) <= cap:
                    code = np.full((n, lpr * epl), WRING_PAD, dtype=np.int64)
                    for p, i in enumerate(rows):
                        for k, j in enumerate(ij[ip[i]:ip[i + 1]]):
                            if j == i:
                                code[p, k] = WRING_DIAG
                            elif level[j] < level[i]:
                                near = level[i] - level[j] <= Wr
                                code[p, k] = pos[j] & ((1 << lg) - 1) if near else WRING_FAR - pos[j]
                            else:
                                code[p, k] = WRING_LATER
                    R.update(path=WRING, wr_lpr=lpr, wr_epl=epl, wr_w=Wr, wr_log2=lg,
                             wr_st=np.array(st, dtype=np.int64).ravel(), wr_code=code.ravel())
        if "NO_WAVE" not in knobs:
            w8 = wave_lpr == 8 if wave_lpr else wide
            lpr = 8 if w8 and max_len <= 64 else 16
            R.update(wave_lpr=lpr, wave_epl=max(1, 1 << ceil_log2(-(-max_len // lpr))))
            if R["path"] is None and deep:
                R["path"] = WAVE
    if R["path"] is None:
        R["path"] = WORKGROUP if deep and mlr <= BLOCK else LEVELS
    return R


def tridiag(n):
    return gc.sorted_csr(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n)))


SMALL = {
    "five_point_12": lambda: gc.sorted_csr(gc.poisson_2d(12)),
    "seven_point_6": lambda: gc.sorted_csr(gc.poisson_3d(6)),
    "nine_point_12": lambda: gc.sorted_csr(gc.nine_point(12)),
    "long_rows_24": lambda: gc.sorted_csr(gc.long_rows(24)),
    "unsorted_zero_diag_16": lambda: gc.unsorted_zero_diag(16),
    "empty": lambda: sp.csr_matrix((0, 0)),
    "one_by_one": lambda: sp.csr_matrix(np.array([[3.0]])),
    "diagonal_7": lambda: sp.identity(7, format="csr"),
    "tridiag_4": lambda: tridiag(4),
    "tridiag_5": lambda: tridiag(5),
}
SMALL_KNOBS = ((), ("NO_WIN",), ("NO_WIN", "NO_RING"), ("NO_WIN", "NO_RING", "NO_LDS"),
               ("NO_WRING",), ("NO_WRING", "NO_WAVE"))


@pytest.mark.parametrize("name", sorted(SMALL))
def test_plan_matches_restatement(driver, tmp_path, name):
    A = SMALL[name]()
    for backward in (False, True):
        for knobs in SMALL_KNOBS:
            S, V = plan(driver, tmp_path, A, backward, knobs)
            R = restate(A, backward, knobs)
            for key, want in R.items():
                got = V[key] if key in V else S[key]
                assert np.array_equal(got, want), (name, backward, knobs, key)
            check_invariants(A, backward, S, V)
    if name == "nine_point_12":
        assert R["n_levels"] > 4 and restate(A)["win_w"] == 3
    if name in ("tridiag_4", "tridiag_5"):  # the n_levels > 4 edge
        assert restate(A)["path"] == (LEVELS if name == "tridiag_4" else WINDOW)


def test_wave_lanes_knob(driver, tmp_path):
    A = gc.band(600, 40)
    for lpr, pair in ((0, (16, 8)), (8, (16, 8)), (16, (16, 8))):  # 81 entries: 16 x 8 only
        S, _ = plan(driver, tmp_path, A, wave_lpr=lpr)
        assert (S["wave_lpr"], S["wave_epl"]) == pair == tuple(
            restate(A, wave_lpr=lpr)[k] for k in ("wave_lpr", "wave_epl"))
    A = gc.sorted_csr(gc.long_rows(24))  # 25 entries, 24 rows a level: 16 x 2, forced 8 x 4
    for lpr, pair in ((0, (16, 2)), (8, (8, 4)), (16, (16, 2))):
        S, _ = plan(driver, tmp_path, A, knobs=("NO_WRING",), wave_lpr=lpr)
        assert (S["wave_lpr"], S["wave_epl"]) == pair


# ---------------------------------------------------------------- invariants
def check_invariants(A, backward, S, V):
    """Properties every plan must have whatever the rules that made it; vectorised."""
    n, ip, ij = A.shape[0], A.indptr.astype(np.int64), A.indices.astype(np.int64)
    level, lp, rows, nlev = V["level"], V["level_ptr"], V["rows"], S["n_levels"]
    assert len(level) == n and len(rows) == n and len(lp) == nlev + 1 and lp[0] == 0
    if n == 0:
        assert nlev == 0 and S["path"] == LEVELS
        return
    # every row in exactly one level, rows ascending within a level
    assert lp[-1] == n and np.all(np.diff(lp) > 0) and np.diff(lp).max() == S["max_level_rows"]
    assert np.array_equal(np.sort(rows), np.arange(n))
    lev_of_pos = np.repeat(np.arange(nlev), np.diff(lp))
    assert np.array_equal(level[rows], lev_of_pos)
    same = lev_of_pos[1:] == lev_of_pos[:-1]
    assert np.all(np.diff(rows)[same] > 0)
    pos = np.empty(n, dtype=np.int64)
    pos[rows] = np.arange(n)
    # coupled rows never share a level; the earlier-swept one has the lower level, and a row's
    # level is one above the highest of its earlier-swept neighbours (0 without any)
    ri = np.repeat(np.arange(n), np.diff(ip))
    off = ri != ij
    a, b = np.concatenate([ri[off], ij[off]]), np.concatenate([ij[off], ri[off]])
    first = (b > a) if backward else (b < a)  # b swept before a
    assert np.all(level[b[first]] < level[a[first]])
    need = np.zeros(n, dtype=np.int64)
    np.maximum.at(need, a[first], level[b[first]] + 1)
    assert np.array_equal(level, need)
    d = level[ri[off]] - level[ij[off]]
    W_earlier, W_both = max(int(d.max(initial=0)), 0), int(np.abs(d).max(initial=0))
    entry_k = np.arange(len(ij)) - np.repeat(ip[:-1], np.diff(ip))  # index within its row
    if S["packed"]:
        K = S["K"]
        pcol = V["pcol"].reshape(n, K)
        assert K in (4, 8) and S["max_level_rows"] <= 2 * BLOCK
        cnt = np.bincount(ri[off], minlength=n)
        assert cnt.max() <= K and np.array_equal((pcol >= 0).sum(axis=1), cnt[rows])
        # stored order of the off-diagonals, pads after them; values and the last diagonal
        slot = np.arange(off.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        assert np.array_equal(pcol[pos[ri[off]], slot], ij[off])
        assert np.array_equal(V["pval"].reshape(n, K)[pos[ri[off]], slot], A.data[off])
        diag = np.zeros(n)
        diag[ri[~off]] = A.data[~off]  # later entries overwrite earlier ones
        assert np.array_equal(V["pdiag"], diag[rows])
    if S["window"]:
        K, cap, lg, nch, W = S["K"], S["win_cap"], S["ring_log2"], S["n_chunks"], S["win_w"]
        assert W == W_both and 1 <= S["win_rw"] <= 8 and S["max_level_rows"] <= 64 * S["win_rw"]
        assert S["win_rw"] == -(-S["max_level_rows"] // 64) and cap <= 4096
        rec, starts = V["clev"][:8 * nch].reshape(nch, 8), V["clev"][8 * nch:]
        l1 = np.cumsum(rec[:, 0])
        l0 = l1 - rec[:, 0]
        assert l1[-1] == nlev and np.all(rec[:, 0] >= 1)  # chunks tile the levels in order
        assert np.array_equal(rec[:, 1], lp[l0]) and np.array_equal(rec[:, 2], lp[l1] - lp[l0])
        assert np.all((rec[:, 2] <= cap) | (rec[:, 0] == 1)) and np.all(rec[:, 2] <= 4096)
        # a chunk's staging buffer and the kernel's registers hold its widest level
        assert S["max_level_rows"] <= cap
        la = np.where(np.arange(nch) == 0, 0, np.minimum(nlev, l0 + W))
        lb = np.minimum(nlev, l1 + W)
        assert np.array_equal(rec[:, 3], lp[la]) and np.array_equal(rec[:, 4], lp[lb] - lp[la])
        assert np.array_equal(rec[:, 5], np.cumsum(rec[:, 0] + 1) - rec[:, 0] - 1)
        want = np.concatenate([lp[x:y + 1] - lp[x] for x, y in zip(l0, l1)])
        assert np.array_equal(starts, want)
        # live together: a chunk's levels and the next one's being staged, W levels either side
        nxt = np.concatenate([l1[1:], [nlev]])
        live = lp[np.minimum(nlev, nxt + W)] - lp[np.maximum(0, l0 - W)]
        assert live.max() <= 1 << lg <= 1 << 15  # slots are uint16, 2^lg the zero slot
        assert ((1 << lg) + 4) * 8 + 2 * win_buf_bytes(cap, K) <= S["win_lds"] <= BUDGET + 64
        pcol = V["pcol"]
        assert np.array_equal(V["wcol"], np.where(pcol >= 0, pos[np.maximum(pcol, 0)], -1))
    if S["ring"]:
        lg, W = S["ring_log2_r"], S["ring_w"]
        assert S["K"] == 4 and S["max_level_rows"] <= BLOCK and W == W_earlier
        assert widest_span(lp, W) <= 1 << lg <= 1 << RING_MAX_LOG2
        assert 8 * ((1 << lg) + 1) + 4 * (nlev + 1) == S["ring_lds"] <= BUDGET
        pcol, code, rcol = V["pcol"], V["rcode"], V["rcol"]
        c = np.maximum(pcol, 0)
        earlier = (pcol >= 0) & (level[c] < np.repeat(lev_of_pos, 4))
        later = (pcol >= 0) & ~earlier
        assert np.all(code[pcol < 0] == RING_PAD) and np.all(rcol[pcol < 0] == -1)
        assert np.all(code[later] == RING_LATER) and np.array_equal(rcol[later], -(pcol[later] + 2))
        assert np.array_equal(code[earlier], pos[c[earlier]] & ((1 << lg) - 1))
        assert np.array_equal(rcol[earlier], pos[c[earlier]]) and np.all(code[earlier] < RING_LATER)
    if S["wring"]:
        lpr, epl, lg, Wr = S["wr_lpr"], S["wr_epl"], S["wr_log2"], S["wr_w"]
        span, rps = lpr * epl, (1024 if epl == 2 else 512) // lpr
        assert lpr in (8, 16) and epl in (2, 4) and S["max_len"] <= span
        st = V["wr_st"].reshape(-1, 2)
        # steps tile the positions in order, each inside one level, at most rows_per_step rows
        assert st[0, 0] == 0 and np.all(st[:, 1] >= 1) and np.all(st[:, 1] <= rps)
        assert np.array_equal(st[:, 0] + st[:, 1], np.concatenate([st[1:, 0], [n]]))
        assert np.array_equal(lev_of_pos[st[:, 0]], lev_of_pos[st[:, 0] + st[:, 1] - 1])
        assert len(st) <= 2 * nlev
        assert np.array_equal(V["wr_len"], np.diff(ip)[rows])
        assert widest_span(lp, Wr) <= 1 << lg <= 1 << RING_MAX_LOG2
        assert Wr == W_earlier or Wr >= 2  # far values are gathered two steps ahead
        assert 8 * ((1 << lg) + 3) + 10 * rps * span + 8 + 8 * len(st) <= S["wr_lds"] <= BUDGET
        code = V["wr_code"].reshape(n, span)
        got = code[pos[ri], entry_k]
        dist = level[ri] - level[ij]
        near, far = off & (dist > 0) & (dist <= Wr), off & (dist > Wr)
        assert np.all(got[~off] == WRING_DIAG) and np.all(got[off & (dist < 0)] == WRING_LATER)
        assert np.array_equal(got[near], pos[ij[near]] & ((1 << lg) - 1))
        assert np.array_equal(got[far], WRING_FAR - pos[ij[far]]) and np.all(got[far] <= WRING_FAR)
        assert (code != WRING_PAD).sum() == len(ij)
    if S["wave"]:
        wpos = V["wpos"].reshape(n, 4)
        assert np.array_equal(wpos[:, 0], rows) and np.array_equal(wpos[:, 1], ip[rows])
        assert np.array_equal(wpos[:, 2], np.diff(ip)[rows]) and not wpos[:, 3].any()
        assert S["wave_lpr"] in (8, 16) and S["wave_epl"] in (1, 2, 4, 8)
        assert S["max_len"] <= S["wave_lpr"] * S["wave_epl"]
    # the path is one of the planned candidates, and only where its kernel's limits hold
    path, deep = S["path"], nlev > 4
    assert {WINDOW: S["window"], RING: S["ring"], PIPE_LDS: S["pipe_lds"], PIPE: S["packed"],
            WRING: S["wring"], WAVE: S["wave"], WORKGROUP: True, LEVELS: True}[path]
    if path != LEVELS:
        assert deep and S["max_level_rows"] <= {
            WINDOW: 512, RING: BLOCK, PIPE_LDS: BLOCK, PIPE: 2 * BLOCK, WRING: BLOCK_MAX_LEVEL_ROWS,
            WAVE: BLOCK_MAX_LEVEL_ROWS, WORKGROUP: BLOCK}[path]
    if path == PIPE_LDS:
        assert n <= LDS_MAX


# ---------------------------------------------------------------- the path table
TABLE = [(name, build, (), path) for name, (build, path) in gc.BOTH_SCHEDULES.items()]
TABLE += [(name, build, knobs, path) for name, (build, knobs, path) in gc.EVERY_PATH.items()]
TABLE += [
    ("grid_600", lambda: gc.sorted_csr(gc.poisson_2d(600)), (), RING),
    ("long_rows_24", lambda: gc.sorted_csr(gc.long_rows(24)), (), WRING),
    ("tridiag_4", lambda: tridiag(4), (), LEVELS),
]


@pytest.mark.parametrize("name,build,knobs,path", TABLE, ids=[t[0] for t in TABLE])
def test_path_table_and_invariants(driver, tmp_path, name, build, knobs, path):
    """Every matrix of the GPU sweeps' tests at its real size, both directions: the path of the
    table and the invariants (the matrices are structurally symmetric under i -> n-1-i up to
    boundary rows, and both directions take the same path)."""
    A = build()
    for backward in (False, True):
        S, V = plan(driver, tmp_path, A, backward, knobs)
        assert gc.PATH_NAMES[S["path"]] == gc.PATH_NAMES[path], (name, backward)
        check_invariants(A, backward, S, V)
    if name in ("grid_1100", "pipe_r2_slab_1500"):
        assert S["K"] == 4 and BLOCK < S["max_level_rows"] <= 2 * BLOCK  # R = 2
    if name.startswith("pipe_r1") or name.startswith("lds_"):
        assert S["K"] == (8 if "k8" in name else 4) and S["max_level_rows"] <= BLOCK
    if name in ("long_rows", "long_rows_24"):
        assert (S["wr_lpr"], S["wr_epl"]) == (16, 2)
    if name == "pipe_r2_slab_1500":
        assert S["n_levels"] == 6 and S["max_level_rows"] == 1500
    if name == "ring_slab_600":
        assert S["max_level_rows"] == 600
