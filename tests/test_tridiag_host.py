"""The bisection of the Lanczos driver (csrc/tridiag.hpp: sturm_count, tridiag_max_eig) on the
CPU: compiled with g++ together with tests/host/tridiag_driver.cpp, once plainly and once with
the address and undefined-behaviour sanitizers, and compared with LAPACK
(scipy.linalg.eigvalsh_tridiagonal) on the inputs where a Sturm sequence goes wrong: one and two
rows, decoupled rows, a pivot of exactly zero, off-diagonals whose squares underflow, the zero
matrix, negative spectra, a diagonal graded over 16 decades, long random matrices and a Lanczos
T with ghost copies of its converged eigenvalues. mlamg.dsetup's Python copy of the same two
routines runs over the same inputs.

The bound is |theta - lambda_max| <= 4 eps ||T||_inf: a Sturm count is exact for a matrix within
a small multiple of eps ||T|| of T, and the bisection ends one ulp wide."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.linalg import eigvalsh_tridiagonal

import lanczos_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml-amg_amd", "csrc")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module", params=("plain", "sanitized"))
def driver(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("tridiag") / f"driver_{request.param}")
    flags = ["-O1"]
    if request.param == "sanitized":
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([cxx, "-std=c++17", *flags, f"-I{CSRC}",
                        os.path.join(ROOT, "tests", "host", "tridiag_driver.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and request.param == "sanitized" and any(
            w in r.stderr for w in ("-lasan", "-lubsan", "libasan", "libubsan")):
        pytest.skip("the sanitizer runtime is not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    return exe


def _inputs():
    """name -> (a[m], off[m - 1]): diagonal and off-diagonal."""
    T = {
        "one_row": ([3.5], []),
        "one_row_negative": ([-2.0], []),
        "two_rows": ([1.0, 3.0], [2.0]),
        "two_rows_equal": ([2.0, 2.0], [1.0]),
        "decoupled_9": (np.linspace(-1.0, 4.0, 9)[::-1].copy(), np.zeros(8)),
        "decoupled_equal_5": (np.full(5, 1.25), np.zeros(4)),
        # Gershgorin gives [0, 4] and the first midpoint is the diagonal itself: q == 0 at row 0
        "toeplitz_7": (np.full(7, 2.0), np.full(6, 1.0)),
        "toeplitz_64": (np.full(64, 2.0), np.full(63, 1.0)),
        "tiny_offdiagonals": (np.linspace(1.0, 2.0, 12), np.full(11, 1e-200)),
        "all_zero_6": (np.zeros(6), np.zeros(5)),
        "negative_20": (np.full(20, -2.0), np.full(19, 1.0)),
        "negative_graded_15": (-10.0 ** np.linspace(-3, 3, 15), np.full(14, 1e-3)),
    }
    a = 10.0 ** np.linspace(-8, 8, 60)
    T["graded_16_decades"] = (a, 0.3 * np.sqrt(a[:-1] * a[1:]))
    T["graded_16_decades_down"] = (a[::-1].copy(), 0.3 * np.sqrt(a[:-1] * a[1:])[::-1].copy())
    for seed in range(3):
        rs = np.random.RandomState(seed)
        T[f"random_400_{seed}"] = (rs.normal(0, 1, 400), rs.normal(0, 1, 399))
    # a Lanczos T run past n steps: 160 rows for a 64-row matrix, so most eigenvalues are ghosts
    _, iters, ha, hb, m = lm.lanczos(lm.matrix("jump1d_64"))
    assert m == iters == 160
    T["lanczos_ghosts_160"] = (np.array(ha), np.array(hb[1:iters]))
    return {k: (np.asarray(a, dtype=np.float64), np.asarray(o, dtype=np.float64))
            for k, (a, o) in T.items()}


INPUTS = _inputs()


def _spectrum(a, off):
    return eigvalsh_tridiagonal(a, off) if len(a) > 1 else a.copy()


def _norm_inf(a, off):
    r = np.abs(a)
    r[1:] += np.abs(off)
    r[:-1] += np.abs(off)
    return float(r.max())


def _queries(ev, norm):
    """Up to 10 points that LAPACK's rounding cannot move across an eigenvalue: below and above
    the spectrum and in the widest gaps, with the number of eigenvalues below each."""
    pad = max(norm, 1.0)
    xs = [ev[0] - pad, ev[-1] + pad]
    gaps = np.diff(ev)
    for i in np.argsort(gaps)[::-1][:8]:
        if gaps[i] > 1e-6 * pad:
            xs.append(0.5 * (ev[i] + ev[i + 1]))
    xs = np.array(xs)
    return xs, np.array([(ev < x).sum() for x in xs])


@pytest.fixture(scope="module")
def results(driver, tmp_path_factory):
    """One run of the driver over every input -> name -> (theta, counts)."""
    d = tmp_path_factory.mktemp("io")
    fin, fout = d / "in.bin", d / "out.bin"
    expect = {}
    with open(fin, "wb") as f:
        np.asarray([len(INPUTS)], dtype=np.int32).tofile(f)
        for name, (a, off) in INPUTS.items():
            ev = _spectrum(a, off)
            xs, counts = _queries(ev, _norm_inf(a, off))
            expect[name] = (ev[-1], xs, counts)
            np.asarray([len(a), len(xs)], dtype=np.int32).tofile(f)
            a.tofile(f)
            np.concatenate([[0.0], off]).tofile(f)
            xs.tofile(f)
    r = subprocess.run([driver, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    assert r.stdout.split() == ["matrices", str(len(INPUTS))]
    raw = np.fromfile(fout, dtype=np.float64)
    got, at = {}, 0
    for name in INPUTS:
        nq = len(expect[name][1])
        got[name] = (raw[at], raw[at + 1:at + 1 + nq])
        at += 1 + nq
    assert at == len(raw)
    return got, expect


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_max_eig_and_counts_vs_lapack(results, name):
    got, expect = results
    a, off = INPUTS[name]
    theta, counts = got[name]
    ref, _, want = expect[name]
    assert abs(theta - ref) <= 4 * EPS * _norm_inf(a, off), (name, theta, ref)
    assert np.array_equal(counts, want), (name, counts, want)


def test_special_values(results):
    got, _ = results
    assert got["one_row"][0] == 3.5 and got["one_row_negative"][0] == -2.0
    assert got["all_zero_6"][0] == 0.0 and got["decoupled_equal_5"][0] == 1.25
    # the ghosts are there: 160 eigenvalues for a 64-row matrix, most of them repeated copies
    a, off = INPUTS["lanczos_ghosts_160"]
    ev = _spectrum(a, off)
    assert (np.diff(ev) < 1e-10).sum() >= 50
    assert abs(got["lanczos_ghosts_160"][0] - lm.reference("jump1d_64")) <= 1e-12 * ev[-1]


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_python_copy_of_dsetup(name):
    """mlamg.dsetup._tridiag_max_eig and _sturm_count, the distributed setup's copy."""
    from mlamg import dsetup
    a, off = INPUTS[name]
    b = [0.0] + list(off)
    ev = _spectrum(a, off)
    norm = _norm_inf(a, off)
    theta = dsetup._tridiag_max_eig(list(a), b, len(a))
    assert abs(theta - ev[-1]) <= 4 * EPS * norm, (name, theta, ev[-1])
    assert theta == lm.tridiag_max_eig(list(a), b, len(a))
    xs, want = _queries(ev, norm)
    assert [dsetup._sturm_count(list(a), b, len(a), x) for x in xs] == list(want)
