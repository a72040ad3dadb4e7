"""GPU: mlamg_lambda_max_dinvA (csrc/eig.hip), the Lanczos behind every smoothed-aggregation
weight omega = (4/3)/lambda_max(D^-1 A), where Lanczos is slow or its stop logic decides the
answer. The cases, their exact references (LAPACK on D^-1/2 A D^-1/2, closed forms for 1D
Poisson) and the CPU checks of both are in tests/lanczos_model.py and
tests/test_lambda_max_host.py; the bound is the project's 1e-12 relative, at the default
tol = 1e-15 and seeds 0 to 3.

* 1D diffusion with jumps over four decades (n = 64, 150): orthogonality is lost long before n
  steps and the top eigenvalue settles only after 160 and 480 of them. A routine capped at n
  steps is 1e-5 off here.
* 1D Poisson at n = 2000 (about n steps: many reads of T), n = 33 and 65 (one past a read),
  n = 1, 2, 3, 5 (the Krylov space ends after n steps) and a diagonal matrix (breakdown at
  step 1).
* multiplicity 4, a cluster of three within 1e-6 of the top, Galerkin operators with wide rows,
  unsorted columns and a diagonal stored in two pieces.
* properties: storage formats, repeatability, loose tolerances, diagonals that must be refused.
"""
import ctypes

import pytest

import lanczos_model as lm
from lanczos_model import BOUND

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2, 3)
STORED_AS_IS = ("reversed_columns_64", "split_diagonal_144")  # no canonicalisation on upload


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.graph
    import mlamg.hierarchy
    import mlamg.multigrid
    import mlamg.sparse
    import mlamg.strength
    return mlamg


def upload(ml, name):
    return ml.sparse.DeviceCSR.from_scipy(lm.matrix(name), check=name not in STORED_AS_IS)


def rel(lam, ref):
    return abs(lam - ref) / ref


# ---------------------------------------------------------------- the bound
@pytest.mark.parametrize("name", sorted(lm.CASES))
def test_lambda_max_exact(ml, name):
    """Every case, seeds 0 to 3: within 1e-12 of the exact value; the same bits when asked
    twice; omega = (4/3)/lambda through sa_omega."""
    Ad, ref = upload(ml, name), lm.reference(name)
    n = Ad.shape[0]
    for seed in SEEDS:
        lam, its = ml.multigrid.lambda_max_dinv_a(Ad, seed=seed)
        print(f"{name} n={n} seed={seed}: lam={lam!r} ref={ref!r} rel={rel(lam, ref):.2e} "
              f"iters={its}")
        assert rel(lam, ref) <= BOUND, (name, seed, lam, ref, its)
        assert (lam, its) == ml.multigrid.lambda_max_dinv_a(Ad, seed=seed)
        if name in lm.POISSON_1D:
            assert rel(lam, lm.poisson_closed_form(lm.POISSON_1D[name])) <= BOUND
        if name == "diagonal_40":
            assert its == lm.CHECK  # breakdown at step 1, found at the first read of T
        if name in lm.TINY:
            # beta_n is rounding noise: under the breakdown threshold (stop at the first read)
            # or just over it, and then T grows on with copies until the second read
            assert its in (lm.CHECK, 2 * lm.CHECK)
    assert rel((4.0 / 3.0) / ml.multigrid.sa_omega(Ad), ref) <= BOUND


@pytest.mark.parametrize("name", ("jump1d_64", "jump1d_150"))
def test_jump_cases_run_past_n_steps(ml, name):
    Ad = upload(ml, name)
    its = [ml.multigrid.lambda_max_dinv_a(Ad, seed=seed)[1] for seed in SEEDS]
    print(f"{name}: steps by seed {its}")
    assert min(its) > Ad.shape[0]
    # max_iter is still honoured, and is the old cap when it equals n: far outside the bound
    lam, it = ml.multigrid.lambda_max_dinv_a(Ad, max_iter=Ad.shape[0])
    print(f"{name}: stopped at n steps rel={rel(lam, lm.reference(name)):.2e}")
    assert it == Ad.shape[0] and rel(lam, lm.reference(name)) > 1e-9


# ---------------------------------------------------------------- storage formats
EXACT_FORMATS = ("sell", "sorted", "sell_dict", "long", "rowpat")


@pytest.mark.parametrize("name", ("galerkin_p2d48_L0", "galerkin_p2d48_L1", "poisson1d_2000",
                                  "jump1d_150", "galerkin_jump2d48_L1"))
def test_storage_formats(ml, name):
    """The exact formats give csr_stream's bits (lambda and steps); 'vector', whose products are
    summed in another order, stays within the bound. A format that does not apply to a matrix
    refuses it (EUNSUPPORTED); on the five-point Poisson matrix every one applies."""
    from mlamg._lib import MLAMG_EUNSUPPORTED, MlamgError
    Ad, ref = upload(ml, name), lm.reference(name)
    base = ml.multigrid.lambda_max_dinv_a(Ad.set_format("csr_stream"))
    accepted = []
    for fmt in EXACT_FORMATS:
        try:
            Ad.set_format(fmt)
        except MlamgError as e:
            assert e.code == MLAMG_EUNSUPPORTED, (fmt, e)
            continue
        assert Ad.get_format()[0] == fmt
        accepted.append(fmt)
        assert ml.multigrid.lambda_max_dinv_a(Ad) == base, (name, fmt)
    print(f"{name}: exact formats accepted {accepted}")
    assert {"sell", "sorted"} <= set(accepted)
    if name == "galerkin_p2d48_L0":
        assert {"sell_dict", "rowpat"} <= set(accepted)
    lam, _ = ml.multigrid.lambda_max_dinv_a(Ad.set_format("vector"))
    assert Ad.get_format()[0] == "vector" and rel(lam, ref) <= BOUND


# ---------------------------------------------------------------- loose tolerances
@pytest.mark.parametrize("name", ("jump1d_64", "jump1d_150", "poisson1d_2000",
                                  "galerkin_p2d48_L0", "galerkin_jump2d48_L1",
                                  "top_cluster_200"))
def test_loose_tolerances(ml, name):
    """tol = 1e-8 and 1e-6, the values mlamg/hierarchy.py passes: a Ritz value cannot exceed
    lambda_max beyond rounding, and the steps do not grow as tol loosens. No lower bound is
    asserted: the stop test is a stagnation test, not an error bound."""
    Ad, ref = upload(ml, name), lm.reference(name)
    its = []
    for tol in (1e-15, 1e-8, 1e-6):
        lam, it = ml.multigrid.lambda_max_dinv_a(Ad, tol=tol)
        print(f"{name} tol={tol:g}: rel={(lam - ref) / ref:+.2e} iters={it}")
        assert lam <= ref * (1 + BOUND), (name, tol, lam, ref)
        its.append(it)
    assert its[0] >= its[1] >= its[2], its


# ---------------------------------------------------------------- refused diagonals
def _raw_call(ml, Ad):
    """The C entry itself -> (status, lambda slot, steps slot, message), slots preset."""
    from mlamg import _lib
    lam, its = ctypes.c_double(-123.25), ctypes.c_int(-7)
    rc = _lib.lib.mlamg_lambda_max_dinvA(Ad.handle, 20000, 1e-15, 0, ctypes.byref(lam),
                                         ctypes.byref(its), _lib.stream_ptr())
    msg = _lib.lib.mlamg_last_error()
    return rc, lam.value, its.value, (msg.decode() if msg else "")


@pytest.mark.parametrize("n", (40, 3000))  # one block and several
@pytest.mark.parametrize("kind,word", (("zero", "zero"), ("missing", "no stored"),
                                       ("mixed_sign", "negative"), ("nan", "non-finite")))
def test_bad_diagonal_is_an_error(ml, kind, word, n):
    """A zero, missing, negative or non-finite diagonal entry: MLAMG_EINVAL naming the kind of
    row, the caller's lambda and steps untouched, no NaN handed on as a weight."""
    from mlamg._lib import MLAMG_EINVAL, MlamgError
    good = lm.poisson_1d(n)
    Ad = ml.sparse.DeviceCSR.from_scipy(lm.BAD_DIAGONALS[kind](good), check=False)
    rc, lam, its, msg = _raw_call(ml, Ad)
    assert rc == MLAMG_EINVAL and (lam, its) == (-123.25, -7), (rc, lam, its, msg)
    assert word in msg and "diagonal" in msg, msg
    with pytest.raises(MlamgError):
        ml.multigrid.sa_omega(Ad)
    # and the next call is served as usual
    lam, _ = ml.multigrid.lambda_max_dinv_a(good)
    assert rel(lam, lm.poisson_closed_form(n)) <= BOUND


def test_all_negative_diagonal(ml):
    """-A: either lambda_max(D^-1 A) of A itself, D^-1 A being unchanged, or the same error."""
    from mlamg._lib import MLAMG_EINVAL, MLAMG_OK
    A = lm.matrix("poisson1d_65")
    Ad = ml.sparse.DeviceCSR.from_scipy(lm.BAD_DIAGONALS["all_negative"](A), check=False)
    rc, lam, its, msg = _raw_call(ml, Ad)
    if rc == MLAMG_OK:
        assert rel(lam, lm.reference("poisson1d_65")) <= BOUND
    else:
        assert rc == MLAMG_EINVAL and (lam, its) == (-123.25, -7) and "negative" in msg, msg
