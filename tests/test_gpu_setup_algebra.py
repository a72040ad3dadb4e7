"""Setup algebra of csrc/spgemm.hip at its edges, bit for bit against scipy's own expressions:
mlamg_transpose (A.T.tocsr()), mlamg_spgemm (A @ B, scipy's stored column order), mlamg_galerkin
((P.T @ A @ P).tocsr(), sorted, zeros eliminated) through the sorted expand-sort-compress path,
the dense LDS-row path and the unforced choice between them, mlamg_csr_scale_rows,
mlamg_sa_smoother and mlamg_strength. Every comparison is indptr, indices and the value BITS.

The unmarked tests run without a device: they prove that each input carries the edge it is named
for (chunk-aligned and chunk-spanning runs of equal sort keys for k_run_sums, long rows and a
cancelling first column for k_compress, the `heavy` rule of spgemm_impl both ways) and that
the row-scaling rules documented in spgemm.hip are scipy's on these inputs. The tests marked gpu
run the same inputs through the kernels."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

CHUNK = 2048            # k_run_sums: sorted products staged per workgroup
DENSE_MAX_COLS = 15360  # kDenseMaxCols: widest product k_dense_rows takes (120 KiB of LDS)
DENSE_MAX_CELLS = 1 << 28
DENORMAL = 5e-324


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def ml(torch_cuda):
    import mlamg.hierarchy
    import mlamg.sparse
    return mlamg


# ---------------------------------------------------------------- helpers
def wide(rs, n):
    """Nonzero values over 13 decades: a sum taken in another order changes bits."""
    return rs.randn(n) * 10.0 ** rs.randint(-6, 7, n)


def shuffled_rows(A, rs):
    """A copy of CSR A with the stored order of every row permuted."""
    A = A.tocsr()
    ij, ax = A.indices.copy(), A.data.copy()
    for r in range(A.shape[0]):
        a, b = A.indptr[r], A.indptr[r + 1]
        p = a + rs.permutation(b - a)
        ij[a:b], ax[a:b] = A.indices[p], A.data[p]
    return sp.csr_matrix((ax, ij, A.indptr.copy()), shape=A.shape)


def set_entry(A, r, c, v):
    """Overwrite the stored entry (r, c) of CSR A, which must exist exactly once."""
    k = A.indptr[r] + np.flatnonzero(A.indices[A.indptr[r]:A.indptr[r + 1]] == c)
    assert len(k) == 1, (r, c)
    A.data[k[0]] = v


def pattern(M):
    M = M.tocsr()
    return sp.csr_matrix((np.ones(M.nnz, dtype=np.int64), M.indices.copy(), M.indptr.copy()),
                         shape=M.shape)


def product_runs(A, B):
    """Run lengths and run start offsets of the product stream of A @ B sorted by (row, column):
    every stored A_ik meets every stored B_kj, explicit zeros included."""
    C = (pattern(A) @ pattern(B)).tocsr()
    C.sort_indices()
    lengths = C.data.astype(np.int64)
    return lengths, np.cumsum(lengths) - lengths


def row_products(A, B):
    """Products per row of A @ B."""
    return pattern(A) @ np.diff(B.tocsr().indptr).astype(np.int64)


def assert_same_bits(got, ref):
    ref = ref.tocsr()
    assert got.shape == ref.shape
    assert np.array_equal(got.indptr, ref.indptr)
    assert np.array_equal(got.indices, ref.indices)
    gd = np.ascontiguousarray(got.data, dtype=np.float64).view(np.uint64)
    rd = np.ascontiguousarray(ref.data, dtype=np.float64).view(np.uint64)
    assert np.array_equal(gd, rd)


def upload(ml, A):
    return ml.sparse.DeviceCSR.from_scipy(A)


def sorted_path_ms():
    """Wall time the sorted (expand-sort-compress) SpGEMM has accumulated since the last call;
    0.0 exactly when no product took that path."""
    from mlamg._lib import call
    buf = (ctypes.c_double * 8)()
    call("mlamg_setup_phase_times", buf, 8, 1)
    return float(sum(buf))


# ---------------------------------------------------------------- Galerkin inputs
def arrow(seed, tiny, big, pairs):
    """Diagonal plus one dense row and column (node 0); aggregates: `tiny` single nodes (node 0
    the first), one of `big` nodes, then `pairs` of two nodes. Both Galerkin products then hold
    a run of `big` equal keys, and the tiny aggregates in front of it set where it starts.
    Pair 0 cancels exactly in R @ A, pair 1 in (R A) @ P."""
    rs = np.random.RandomState(seed)
    n = tiny + big + 2 * pairs
    diag, row, col = wide(rs, n), wide(rs, n), wide(rs, n)
    p = wide(rs, n)
    t0 = tiny + big
    if pairs >= 1:  # M[c, 0] = 1 * 0.5 + 1 * -0.5
        p[t0:t0 + 2], col[t0:t0 + 2] = 1.0, (0.5, -0.5)
    if pairs >= 2:  # A_c[c, c] = (1 * 2) * 1 + (1 * -2) * 1
        p[t0 + 2:t0 + 4], diag[t0 + 2:t0 + 4] = 1.0, (2.0, -2.0)
    i = np.arange(n)
    z = np.zeros(n - 1, dtype=np.int64)
    A = sp.csr_matrix((np.concatenate([diag, row[1:], col[1:]]),
                       (np.concatenate([i, z, i[1:]]), np.concatenate([i, i[1:], z]))),
                      shape=(n, n))
    A.sort_indices()
    agg = np.concatenate([np.arange(tiny), np.full(big, tiny),
                          tiny + 1 + np.repeat(np.arange(pairs), 2)])
    P = sp.csr_matrix((p, agg, np.arange(n + 1)), shape=(n, tiny + 1 + pairs))
    return A, P


def agg_problem(seed, n, nc, per_row=3.0, long_row=True, empty=(), zero_cols=()):
    """A sparse n x n operator (per_row entries a row on average plus the diagonal, one row of
    more than 512 entries where n allows) and a block-aggregate prolongator with a second entry
    in every fifth row. Aggregates in `empty` own no node; the P entries in `zero_cols` are
    stored zeros of both signs. Where n allows, nodes 0 and 1 cancel exactly in R @ A."""
    rs = np.random.RandomState(seed)
    lin = np.unique(rs.randint(0, n * n, size=int(per_row * n)))  # distinct positions
    A = sp.csr_matrix((np.ones(len(lin)), (lin // n, lin % n)), shape=(n, n))
    A = A + sp.eye(n, format="csr")
    if long_row and n > 512:
        L = min(n, 700)
        A = A + sp.csr_matrix((np.ones(L), (np.full(L, n // 3), rs.choice(n, L, replace=False))),
                              shape=(n, n))
    owners = np.array([c for c in range(nc) if c not in empty])
    agg = owners[(np.arange(n) * len(owners)) // n]
    p = wide(rs, n)
    rows, cols, vals = [np.arange(n)], [agg], [p]
    if len(owners) > 1:
        extra = np.arange(0, n, 5)
        nxt = owners[((extra * len(owners)) // n + 1) % len(owners)]
        keep = nxt != agg[extra]
        rows.append(extra[keep]), cols.append(nxt[keep]), vals.append(wide(rs, int(keep.sum())))
    # a column that, within the first aggregate, only nodes 0 and 1 will reach
    first = np.concatenate(rows)[np.concatenate(cols) == owners[0]]
    free = np.flatnonzero(np.asarray(abs(A.tocsr()[first]).sum(axis=0)).ravel() == 0)
    plant = n >= 2 * len(owners) and len(free) > 0
    if plant:
        A = A + sp.csr_matrix((np.ones(2), ([0, 1], [free[0], free[0]])), shape=(n, n))
    A = A.tocsr()
    A.sort_indices()
    A.data[:] = wide(rs, A.nnz)
    if plant:
        p[:2] = 1.0
        set_entry(A, 0, free[0], 0.25)
        set_entry(A, 1, free[0], -0.25)
    P = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(n, nc))
    P.sort_indices()
    for c in zero_cols:
        k = np.flatnonzero(P.indices == c)
        P.data[k] = np.where(np.arange(len(k)) % 2, -0.0, 0.0)
    return A, P


ARROWS = {
    # name: (builder arguments, run kinds claimed for (R @ A, (R A) @ P))
    "arrow_mid": ((1, 990, 5000, 3), ("ad", "ad")),
    "arrow_aligned": ((2, 682, 4096, 2), ("abcd", "ad")),
    "arrow_last": ((3, 500, 5000, 0), ("ad", "ade")),
}
DENSE_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 8192, 8193, 15360, 15361)
SPECIALS = {
    "empty_aggregate": dict(seed=5, n=300, nc=8, empty=(3,)),
    "zero_block": dict(seed=6, n=300, nc=8, zero_cols=(2, 3, 4)),
    "one_aggregate": dict(seed=7, n=300, nc=1),
    "heavy": dict(seed=8, n=4000, nc=4, per_row=20.0, long_row=False),
}


@functools.lru_cache(maxsize=None)
def galerkin_case(name):
    """(A, P, scipy's coarse operator) of a named input; built once, never written to."""
    if name in ARROWS:
        A, P = arrow(*ARROWS[name][0])
    elif name in SPECIALS:
        A, P = agg_problem(**SPECIALS[name])
    else:
        n = int(name[1:])
        A, P = agg_problem(seed=n, n=n, nc=min(n, 29))
    ref = (P.T @ A @ P).tocsr()
    ref.sort_indices()
    ref.eliminate_zeros()
    assert not np.isnan(ref.data).any()
    return A, P, ref


def galerkin_products(A, P):
    """The operands (R, A) and (R A, P) of the two products as the device forms them."""
    R = P.T.tocsr()
    M = (R @ A).tocsr()  # csr_matmat: exact zeros already dropped, as the kernel drops them
    M.sort_indices()
    return (R, A), (M, P)


def run_kinds(lengths, starts):
    """Which of the run kinds a) to e) a sorted product stream holds, k_run_sums cutting it into
    chunks of 2048: a) a run with a head in one chunk and a whole following chunk of non-heads,
    b) a summing run that starts on a chunk's first slot past chunk 0, c) a summing run that
    ends on a chunk's last slot, d) a final partial chunk, e) the last run crossing into it."""
    total = int(lengths.sum())
    ends = starts + lengths
    multi = lengths >= 2
    kinds = set()
    if np.any((lengths >= 2 * CHUNK) & ((starts // CHUNK + 2) * CHUNK <= ends)):
        kinds.add("a")
    if np.any(multi & (starts % CHUNK == 0) & (starts > 0)):
        kinds.add("b")
    if np.any(multi & (ends % CHUNK == 0)):
        kinds.add("c")
    if total % CHUNK:
        kinds.add("d")
        if len(starts) and starts[-1] < (total // CHUNK) * CHUNK:
            kinds.add("e")
    return kinds


def heavy(a, b):
    """spgemm_impl's rule for taking the dense path unforced, from the shapes alone."""
    return a.nnz * (b.nnz / max(b.shape[0], 1)) > 8.0 * a.shape[0] * min(b.shape[1], 2048)


def fits_dense(a, b):
    return b.shape[1] <= DENSE_MAX_COLS and a.shape[0] * b.shape[1] <= DENSE_MAX_CELLS


# ---------------------------------------------------------------- inputs proven on the CPU
@pytest.mark.parametrize("name", sorted(ARROWS))
def test_arrow_inputs_hold_their_runs(name):
    A, P, ref = galerkin_case(name)
    assert A.shape[0] <= 6000
    for (a, b), claimed in zip(galerkin_products(A, P), ARROWS[name][1]):
        lengths, starts = product_runs(a, b)
        assert lengths.max() == ARROWS[name][0][2]  # the aggregate of `big` nodes, one key
        assert set(claimed) <= run_kinds(lengths, starts), (name, run_kinds(lengths, starts))
        if "b" in claimed:  # it is the long run itself that fills whole chunks, first slot to last
            k = int(np.argmax(lengths))
            assert starts[k] > 0 and starts[k] % CHUNK == 0 and lengths[k] % CHUNK == 0
    # the planted pairs cancel: fewer stored results than structural ones
    (R, _), (M, _) = galerkin_products(A, P)
    if ARROWS[name][0][3] >= 1:
        assert M.nnz < (pattern(R) @ pattern(A)).nnz
    if ARROWS[name][0][3] >= 2:
        assert ref.nnz < (pattern(M) @ pattern(P)).nnz


def test_arrow_inputs_cover_every_run_kind():
    seen = set()
    for name in ARROWS:
        A, P, _ = galerkin_case(name)
        for a, b in galerkin_products(A, P):
            seen |= run_kinds(*product_runs(a, b))
    assert seen == set("abcde")


@pytest.mark.parametrize("n", DENSE_SIZES)
def test_dense_size_inputs(n):
    """The fine size is the column count of R @ A; the coarse size keeps the dense scratch
    small; rows of B longer than the dense kernel's 512-thread stride where n allows; the
    planted cancellation is there."""
    A, P, _ = galerkin_case(f"n{n}")
    (R, _), (M, _) = galerkin_products(A, P)
    assert A.shape == (n, n) and R.shape[0] <= 32
    assert fits_dense(R, A) == (n <= DENSE_MAX_COLS) and fits_dense(M, P)
    if n > 512:
        assert np.diff(A.indptr).max() > 512
    if n >= 64:
        assert M.nnz < (pattern(R) @ pattern(A)).nnz


def test_special_inputs():
    A, P, ref = galerkin_case("empty_aggregate")
    assert np.diff(P.T.tocsr().indptr)[3] == 0
    assert np.diff(ref.indptr)[3] == 0 and not np.any(ref.indices == 3)
    A, P, ref = galerkin_case("zero_block")
    Pc = P.tocsc()
    for c in (2, 3, 4):
        blk = Pc.data[Pc.indptr[c]:Pc.indptr[c + 1]]
        assert len(blk) > 2 and not np.any(blk) and np.signbit(blk).any()
        assert np.diff(ref.indptr)[c] == 0 and not np.any(ref.indices == c)
    A, P, ref = galerkin_case("one_aggregate")
    assert P.shape[1] == 1 and ref.shape == (1, 1) and ref.nnz == 1


def test_heavy_rule_both_ways():
    A, P, _ = galerkin_case("heavy")
    for a, b in galerkin_products(A, P):
        assert heavy(a, b) and fits_dense(a, b)
    for name in ARROWS:
        A, P, _ = galerkin_case(name)
        for a, b in galerkin_products(A, P):
            assert not heavy(a, b)


# ---------------------------------------------------------------- mlamg_spgemm inputs
def _stream(A, B, i):
    """Products of row i in csr_matmat's order: A's stored order, then B's row's."""
    out = []
    for k in range(A.indptr[i], A.indptr[i + 1]):
        j = A.indices[k]
        for kk in range(B.indptr[j], B.indptr[j + 1]):
            out.append((int(B.indices[kk]), A.data[k] * B.data[kk]))
    return out


def _random_pair(seed, m, k, n, da, db):
    rs = np.random.RandomState(seed)
    A = sp.random(m, k, density=da, random_state=rs, format="csr")
    B = sp.random(k, n, density=db, random_state=rs, format="csr")
    A.data[:], B.data[:] = wide(rs, A.nnz), wide(rs, B.nnz)
    return shuffled_rows(A, rs), shuffled_rows(B, rs), rs


def _clear_rows(M, rows):
    M = M.tolil()
    for r in rows:
        M[r, :] = 0
    M = M.tocsr()
    M.eliminate_zeros()
    return M


def _spgemm_ragged():
    A, B, rs = _random_pair(11, 257, 120, 256, 0.1, 0.1)
    B = _clear_rows(B, range(0, 120, 3))  # every third row of B empty
    A = _clear_rows(A, (3, 100, 256))     # empty rows of A, the last one included
    A = A.tolil()
    A[5, :] = 0
    for c in (0, 33, 66, 117):            # row 5 meets only empty rows of B
        A[5, c] = 1.5
    A = A.tocsr()
    return shuffled_rows(A, rs), shuffled_rows(B, rs)


def _spgemm_no_products():
    rs = np.random.RandomState(12)
    A = sp.random(40, 30, density=0.3, random_state=rs, format="csr").tolil()
    A[:, 10:] = 0                         # A only meets rows 0..9 of B, all empty
    B = sp.random(30, 50, density=0.3, random_state=rs, format="csr")
    return shuffled_rows(A.tocsr(), rs), shuffled_rows(_clear_rows(B, range(10)), rs)


def _spgemm_long_row():
    """One row of 300 entries against rows of 300 entries: 90000 products, past 16 index bits."""
    rs = np.random.RandomState(13)
    cols = np.concatenate([rs.choice(400, 300, replace=False) for _ in range(300)])
    B = sp.csr_matrix((wide(rs, 300 * 300), cols, np.arange(0, 300 * 300 + 1, 300)),
                      shape=(300, 400))
    A = sp.csr_matrix((wide(rs, 300 + 4),
                       np.concatenate([[7, 2], rs.permutation(300), [299, 0]]),
                       [0, 2, 302, 304]), shape=(3, 300))
    return A, B


def _spgemm_first_cancels():
    """Row 2's first product lands in column 9 and column 9 sums to exactly zero, while the
    columns that appear after it survive; row 4's first column cancels among three terms."""
    A, B, rs = _random_pair(14, 8, 12, 16, 0.5, 0.5)
    A, B = A.tolil(), B.tolil()
    A[2, :], B[3, :], B[6, :] = 0, 0, 0
    A[4, :], B[1, :] = 0, 0
    B[0, 9] = 0                                           # row 0 of B stays out of column 9
    A, B = A.tocsr(), B.tocsr()
    A.eliminate_zeros(), B.eliminate_zeros()

    def with_row(M, r, cols, vals):
        M = M.tocsr()
        ip = M.indptr.copy()
        assert ip[r + 1] == ip[r]
        ij = np.concatenate([M.indices[:ip[r]], cols, M.indices[ip[r]:]]).astype(np.int32)
        ax = np.concatenate([M.data[:ip[r]], vals, M.data[ip[r]:]])
        ip[r + 1:] += len(cols)
        return sp.csr_matrix((ax, ij, ip), shape=M.shape)

    B = with_row(B, 3, [9, 1, 14], [2.0, 3.0, 0.375])
    B = with_row(B, 6, [14, 9, 5], [1.0, 4.0, -7.0])
    B = with_row(B, 1, [0, 9], [8.0, 0.5])
    A = with_row(A, 2, [3, 0, 6], [1.0, 1e-3, -0.5])      # col 9 first: 1 * 2 - 0.5 * 4
    A = with_row(A, 4, [3, 1, 6], [1.0, 4.0, -1.0])       # col 9 first: 2 + 2 - 4
    return A, B


def _spgemm_neg_zero():
    """Products that are -0.0 (a stored zero times a negative, an underflow): 0 + -0.0 is +0.0
    and is dropped; next to them ordinary products in the same rows."""
    A = sp.csr_matrix((np.array([0.0, 3.0, -1e-200, 2.0, -0.0]), np.array([1, 0, 2, 1, 0]),
                       np.array([0, 2, 4, 5])), shape=(3, 3))
    B = sp.csr_matrix((np.array([5.0, -2.0, -4.0, 1e-200, 7.0]), np.array([2, 0, 1, 0, 2]),
                       np.array([0, 2, 3, 5])), shape=(3, 3))
    return A, B


SHAPES = {  # name: (rows of A, inner, columns of B, density of A, density of B)
    "b1col": (64, 50, 1, 0.3, 0.5), "b2col": (256, 64, 2, 0.2, 0.6),
    "b256col": (257, 64, 256, 0.1, 0.1), "b257col": (64, 300, 257, 0.5, 0.1),
    "a1row": (1, 300, 256, 0.5, 0.1), "a1row_b1col": (1, 40, 1, 0.5, 0.5),
}
SPGEMM_CASES = sorted(SHAPES) + ["ragged", "no_products", "long_row", "first_cancels",
                                 "neg_zero"]


@functools.lru_cache(maxsize=None)
def spgemm_case(name):
    if name in SHAPES:
        m, k, n, da, db = SHAPES[name]
        A, B, _ = _random_pair(sum(map(ord, name)), m, k, n, da, db)
    else:
        A, B = globals()["_spgemm_" + name]()
    A, B = A.tocsr(), B.tocsr()
    ref = A @ B
    assert not np.isnan(ref.data).any()
    return A, B, ref


def test_spgemm_inputs():
    counts = {name: row_products(*spgemm_case(name)[:2]) for name in SPGEMM_CASES}
    assert counts["long_row"].max() > 65536
    assert counts["b257col"].max() > 256 and counts["a1row"].max() > 256
    assert (pattern(spgemm_case("b257col")[0]) @ pattern(spgemm_case("b257col")[1])).nnz > 0
    A, B, ref = spgemm_case("no_products")
    assert A.nnz > 0 and B.nnz > 0 and counts["no_products"].sum() == 0 and ref.nnz == 0
    A, B, ref = spgemm_case("ragged")
    assert counts["ragged"][5] == 0 and A.indptr[6] - A.indptr[5] == 4
    assert A.indptr[4] == A.indptr[3] and A.indptr[257] == A.indptr[256]
    for name in sorted(SHAPES) + ["ragged", "long_row"]:  # stored order really is unsorted
        A, B, _ = spgemm_case(name)
        assert not A.has_sorted_indices
        assert not B.has_sorted_indices or B.shape[1] == 1
    A, B, ref = spgemm_case("first_cancels")
    for i in (2, 4):
        s = _stream(A, B, i)
        first = s[0][0]
        acc = 0.0
        for c, v in s:
            if c == first:
                acc += v
        got = ref.indices[ref.indptr[i]:ref.indptr[i + 1]]
        assert acc == 0.0 and sum(c == first for c, _ in s) >= 2 and first not in got
        assert len(got) >= 2
    A, B, ref = spgemm_case("neg_zero")
    prods = [v for i in range(3) for _, v in _stream(A, B, i)]
    assert sum(1 for v in prods if v == 0.0 and np.signbit(v)) >= 2
    assert not np.any(ref.data == 0.0) and 0 < ref.nnz < (pattern(A) @ pattern(B)).nnz


# ---------------------------------------------------------------- transpose inputs
def _special_values(rs, n):
    v = wide(rs, n)
    for k, s in enumerate((-0.0, np.inf, -np.inf, DENORMAL, -DENORMAL, 0.0, 2.5e-310)):
        v[k::11][:3] = s
    return v


def _transpose_random(seed, m, n, density):
    rs = np.random.RandomState(seed)
    A = sp.random(m, n, density=density, random_state=rs, format="csr")
    A.data[:] = _special_values(rs, A.nnz)
    return shuffled_rows(A, rs)


def _transpose_one_column():
    """Column 5 holds every one of 3000 rows (one atomic counter takes them all)."""
    rs = np.random.RandomState(21)
    A = sp.random(3000, 40, density=0.02, random_state=rs, format="lil")
    A[:, 5] = 1.0
    A = A.tocsr()
    A.data[:] = _special_values(rs, A.nnz)
    return shuffled_rows(A, rs)


def _transpose_gaps():
    """Empty rows (first and last among them) and empty columns (first and last among them)."""
    rs = np.random.RandomState(22)
    A = sp.random(300, 70, density=0.05, random_state=rs, format="lil")
    for r in (0, 17, 18, 299):
        A[r, :] = 0
    for c in (0, 33, 69):
        A[:, c] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    A.data[:] = _special_values(rs, A.nnz)
    return shuffled_rows(A, rs)


TRANSPOSE_SHAPES = {f"{m}x{n}": (m, n) for m, n in
                    ((1, 1), (1, 256), (256, 1), (1, 257), (257, 1), (256, 257), (257, 256),
                     (256, 256), (70, 300), (300, 70))}
TRANSPOSE_CASES = sorted(TRANSPOSE_SHAPES) + ["one_column", "gaps", "no_entries"]


@functools.lru_cache(maxsize=None)
def transpose_case(name):
    if name in TRANSPOSE_SHAPES:
        m, n = TRANSPOSE_SHAPES[name]
        return _transpose_random(m * 1000 + n, m, n, 1.0 if min(m, n) == 1 else 0.08)
    if name == "no_entries":
        return sp.csr_matrix((37, 19))
    return globals()["_transpose_" + name]()


def test_transpose_inputs():
    A = transpose_case("one_column")
    assert np.sum(A.indices == 5) == A.shape[0] == 3000
    A = transpose_case("gaps")
    assert np.diff(A.indptr)[[0, 17, 18, 299]].sum() == 0
    assert not np.isin([0, 33, 69], A.indices).any()
    assert transpose_case("no_entries").nnz == 0
    for name in ("256x257", "300x70", "one_column", "gaps"):
        A = transpose_case(name)
        assert not A.has_sorted_indices
        bits = set(A.data.view(np.uint64).tolist())
        for s in (-0.0, np.inf, DENORMAL):
            assert int(np.float64(s).view(np.uint64)) in bits


# ---------------------------------------------------------------- row scaling / smoother inputs
def _scale_input(seed, m, n, unsorted):
    """A with stored zeros of both signs, negative entries and empty rows; d with zeros of both
    signs (on rows holding 0 * negative and -0 * positive), and one row whose products with d_i
    underflow to zeros of both signs. All finite."""
    rs = np.random.RandomState(seed)
    A = _clear_rows(sp.random(m, n, density=0.08, random_state=rs, format="csr"), (5, m - 1))
    A.data[:] = wide(rs, A.nnz)
    A.data[::7] = 0.0
    A.data[3::7] = -0.0
    d = wide(rs, m)
    lens = np.diff(A.indptr)
    full = np.flatnonzero(lens >= 3)
    zero_rows, tiny_row = full[:3], full[3]
    d[zero_rows] = (0.0, -0.0, 0.0)
    A.data[A.indptr[zero_rows[0]]] = -3.0
    A.data[A.indptr[zero_rows[1]] + 1] = 2.0
    d[tiny_row] = 1e-200
    A.data[A.indptr[tiny_row]:A.indptr[tiny_row + 1]] = 3.0
    A.data[A.indptr[tiny_row]:A.indptr[tiny_row] + 2] = (1e-200, -1e-200)
    return (shuffled_rows(A, rs) if unsorted else A), d


SCALE_CASES = {"sorted_square": (31, 200, 200, False), "unsorted_square": (32, 257, 257, True),
               "unsorted_wide": (33, 120, 300, True), "sorted_tall": (34, 300, 90, False),
               "one_row": (35, 1, 256, True)}


@functools.lru_cache(maxsize=None)
def scale_case(name):
    seed, m, n, unsorted = SCALE_CASES[name]
    if name == "one_row":
        rs = np.random.RandomState(seed)
        A = sp.csr_matrix(wide(rs, n).reshape(1, n))
        A.data[::5] = 0.0
        return shuffled_rows(A, rs), np.array([-2.5e-3])
    return _scale_input(seed, m, n, unsorted)


def scale_ref(A, d, reverse):
    if reverse:
        return (sp.diags(d) @ A).tocsr()
    return sp.csr_matrix((A.data * np.repeat(d, np.diff(A.indptr)), A.indices.copy(),
                          A.indptr.copy()), shape=A.shape)


def _sa_input(seed, n, unsorted, omega):
    """Square, diagonal present and nonzero in every row, stored zeros off the diagonal; rows
    3k hold a power-of-two diagonal, so that at omega = 1 their 1 - (1/a)*a is exactly 0."""
    rs = np.random.RandomState(seed)
    A = (sp.random(n, n, density=min(1.0, 5.0 / n), random_state=rs, format="csr")
         + sp.eye(n, format="csr")).tocsr()
    A.sort_indices()
    A.data[:] = wide(rs, A.nnz)
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    off = np.flatnonzero(rows != A.indices)
    A.data[off[::6]] = 0.0
    A.data[off[3::6]] = -0.0
    dg = np.flatnonzero(rows == A.indices)
    A.data[dg[::3]] = 2.0 ** rs.randint(-8, 9, len(dg[::3])) * rs.choice([-1.0, 1.0], len(dg[::3]))
    return (shuffled_rows(A, rs) if unsorted else A), omega


def _sa_diag_places():
    """Four-entry rows with the diagonal stored first, in the middle and last."""
    n = 9
    rs = np.random.RandomState(44)
    ij, ax = [], []
    for i in range(n):
        others = [(i + 1) % n, (i + 4) % n, (i + 7) % n]
        others.insert((0, 1, 2, 3)[i % 4], i)
        ij += others
        ax += list(wide(rs, 4))
    return sp.csr_matrix((np.array(ax), np.array(ij), np.arange(0, 4 * n + 1, 4)),
                         shape=(n, n)), 0.7


def _sa_missing_diagonal():
    """Rows 2 and 5 store no diagonal: scipy's 1/0 scale turns their entries into infinities
    (no stored zero there, so no NaN) and leaves the identity's 1 on the diagonal."""
    A, omega = _sa_input(45, 40, True, 4.0 / 3.0)
    A = A.tolil()
    for r in (2, 5):
        A[r, :] = 0
        A[r, (r + 1) % 40], A[r, (r + 9) % 40] = -1.5, 0.3
    return A.tocsr(), omega


SA_CASES = {
    "sorted": lambda: _sa_input(41, 200, False, 2.0 / 3.0),
    "unsorted": lambda: _sa_input(42, 257, True, 4.0 / 3.0 / 1.9),
    "omega_one": lambda: _sa_input(43, 200, True, 1.0),
    "omega_one_sorted": lambda: _sa_input(46, 64, False, 1.0),
    "diag_places": _sa_diag_places,
    "one_by_one": lambda: (sp.csr_matrix(np.array([[-3.7]])), 0.5),
    "one_by_one_cancels": lambda: (sp.csr_matrix(np.array([[4.0]])), 1.0),
    "missing_diagonal": _sa_missing_diagonal,
}


@functools.lru_cache(maxsize=None)
def sa_case(name):
    A, omega = SA_CASES[name]()
    A = A.tocsr()
    n = A.shape[0]
    with np.errstate(divide="ignore"):
        ref = sp.eye(n) - omega * sp.diags([1.0 / A.diagonal()], [0]) @ A
    return A, omega, ref.tocsr()


def _rule_scale(A, d, mode):
    """The row rules written in spgemm.hip (k_scale_count / k_scale_fill), in numpy: mode 0
    diag(d) @ A in reversed stored order with zeros dropped, mode 1 I - diag(d) @ A in stored
    order without the diagonal, then the diagonal, zeros dropped."""
    ip, ij, ax = [0], [], []
    for i in range(A.shape[0]):
        ks = range(A.indptr[i], A.indptr[i + 1])
        if mode == 0:
            for k in reversed(ks):
                m = d[i] * A.data[k]
                if m != 0.0:
                    ij.append(A.indices[k]), ax.append(m)
        else:
            mdiag = 0.0
            for k in ks:
                m = d[i] * A.data[k]
                if A.indices[k] == i:
                    mdiag = m
                elif 0.0 - m != 0.0:
                    ij.append(A.indices[k]), ax.append(0.0 - m)
            if 1.0 - mdiag != 0.0:
                ij.append(i), ax.append(1.0 - mdiag)
        ip.append(len(ij))
    return sp.csr_matrix((np.array(ax, dtype=np.float64), np.array(ij, dtype=np.int32),
                          np.array(ip, dtype=np.int32)), shape=A.shape)


@pytest.mark.parametrize("name", sorted(SCALE_CASES))
def test_scale_inputs_and_rule(name):
    A, d = scale_case(name)
    ref = scale_ref(A, d, 1)
    assert not np.isnan(ref.data).any() and np.isfinite(A.data).all()
    assert_same_bits(_rule_scale(A, d, 0), ref)
    kept = scale_ref(A, d, 0)
    assert kept.nnz == A.nnz and not np.isnan(kept.data).any()
    if name != "one_row":
        assert np.any(A.data == 0.0) and np.any(d == 0.0) and np.any(np.diff(A.indptr) == 0)
        zr = np.flatnonzero(d == 0.0)
        assert all(np.diff(ref.indptr)[zr] == 0) and np.diff(A.indptr)[zr].min() >= 3
        neg_zero = (kept.data == 0.0) & np.signbit(kept.data)
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        assert np.isin(zr[:2], rows[neg_zero]).all()  # 0 * negative and -0 * positive
        under = (A.data != 0.0) & (np.repeat(d, np.diff(A.indptr)) != 0.0) & (kept.data == 0.0)
        assert under.sum() >= 2  # products that underflow to zero, of both signs
        assert A.has_sorted_indices == (not SCALE_CASES[name][3])


@pytest.mark.parametrize("name", sorted(SA_CASES))
def test_sa_inputs_and_rule(name):
    A, omega, ref = sa_case(name)
    assert not np.isnan(ref.data).any()
    with np.errstate(divide="ignore"):
        d = (1.0 / A.diagonal()) * omega
    assert_same_bits(_rule_scale(A, d, 1), ref)
    n = A.shape[0]
    has_diag = np.array([i in ref.indices[ref.indptr[i]:ref.indptr[i + 1]] for i in range(n)])
    if name.startswith("omega_one") or name == "one_by_one_cancels":
        assert omega == 1.0 and not has_diag[::3].any()  # the cancelled diagonal is absent
    if name == "missing_diagonal":
        assert np.isinf(ref.data).sum() == 4 and has_diag[[2, 5]].all()
    if name == "diag_places":
        where = [list(A.indices[4 * i:4 * i + 4]).index(i) for i in range(n)]
        assert set(where) == {0, 1, 2, 3}
    if name in ("sorted", "unsorted", "omega_one"):
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        assert np.any((A.data == 0.0) & (rows != A.indices)) and ref.nnz < A.nnz


def strength_input():
    rs = np.random.RandomState(51)
    A = sp.random(257, 300, density=0.05, random_state=rs, format="csr")
    A.data[:] = wide(rs, A.nnz)
    A.data[::2] *= -1.0
    A.data[1::9] = -0.0
    A.data[2::9] = DENORMAL
    A.data[4::9] = -DENORMAL
    A.data[5::9] = 0.0
    return shuffled_rows(A, rs)


# ================================================================ device tests
MODES = ("esc", "dense", None)


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("MLAMG_SPGEMM", raising=False)
    else:
        monkeypatch.setenv("MLAMG_SPGEMM", mode)


def device_galerkin(ml, A, P):
    Ad, Pd = upload(ml, A), upload(ml, P)
    return ml.sparse.galerkin(Pd.transpose(), Ad, Pd).to_scipy()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(ARROWS))
def test_galerkin_long_runs(ml, monkeypatch, name, mode):
    """Runs of equal keys that start on, end on and span k_run_sums' 2048-product chunks
    (test_arrow_inputs_hold_their_runs), through the sorted path, the dense path (R @ A at
    about 6000 columns with a 6000-entry row of B) and whichever the rule picks."""
    _set_mode(monkeypatch, mode)
    A, P, ref = galerkin_case(name)
    sorted_path_ms()
    assert_same_bits(device_galerkin(ml, A, P), ref)
    took_sorted = sorted_path_ms() > 0.0
    assert took_sorted == (mode != "dense")  # unforced: not heavy (test_heavy_rule_both_ways)


@pytest.mark.gpu
@pytest.mark.parametrize("n", DENSE_SIZES)
def test_galerkin_dense_sizes(ml, monkeypatch, n):
    """k_dense_rows at column counts around its 512 / 256 strides, at one and two columns, above
    64 KiB of LDS and at its cap; one column past the cap the forced dense path must quietly
    take the sorted one for R @ A."""
    _set_mode(monkeypatch, "dense")
    A, P, ref = galerkin_case(f"n{n}")
    sorted_path_ms()
    assert_same_bits(device_galerkin(ml, A, P), ref)
    assert (sorted_path_ms() > 0.0) == (n > DENSE_MAX_COLS)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("empty_aggregate", "zero_block", "one_aggregate", "n513",
                                  "n8193"))
def test_galerkin_special_shapes(ml, monkeypatch, name, mode):
    """An aggregate without nodes, a block of P columns holding only stored zeros of both
    signs, a single aggregate, and two of the dense sizes: the same bits on every path."""
    _set_mode(monkeypatch, mode)
    A, P, ref = galerkin_case(name)
    assert_same_bits(device_galerkin(ml, A, P), ref)


@pytest.mark.gpu
def test_galerkin_unforced_heavy(ml, monkeypatch):
    """With the variable unset the rule sends both products of the heavy input to the dense
    path (test_heavy_rule_both_ways) and the result is scipy's."""
    _set_mode(monkeypatch, None)
    A, P, ref = galerkin_case("heavy")
    sorted_path_ms()
    assert_same_bits(device_galerkin(ml, A, P), ref)
    assert sorted_path_ms() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("esc", "dense"))
def test_galerkin_scratch_reuse(ml, monkeypatch, mode):
    """The setup scratch pool hands back uncleared blocks of up to twice the request: a small
    problem, the largest, and the small one again give the same bits."""
    _set_mode(monkeypatch, mode)
    small, large = galerkin_case("empty_aggregate"), galerkin_case("arrow_mid")
    first = device_galerkin(ml, *small[:2])
    assert_same_bits(device_galerkin(ml, *large[:2]), large[2])
    again = device_galerkin(ml, *small[:2])
    assert_same_bits(first, small[2])
    assert_same_bits(again, small[2])
    assert_same_bits(again, first)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SPGEMM_CASES)
def test_spgemm_scipy_order(ml, name):
    """A_dev @ B_dev with unsorted rows on both sides: scipy's values, zero dropping and stored
    column order (k_compress, order 1)."""
    A, B, ref = spgemm_case(name)
    assert_same_bits((upload(ml, A) @ upload(ml, B)).to_scipy(), ref)


@pytest.mark.gpu
def test_spgemm_scratch_reuse(ml):
    small, large = spgemm_case("first_cancels"), spgemm_case("long_row")
    for A, B, ref in (small, large, small):
        assert_same_bits((upload(ml, A) @ upload(ml, B)).to_scipy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TRANSPOSE_CASES)
def test_transpose(ml, name):
    """A.T.tocsr() with every value carried bit for bit (-0.0, infinities, denormals), and the
    transpose of that is the row-sorted original."""
    A = transpose_case(name)
    Td = upload(ml, A).transpose()
    assert_same_bits(Td.to_scipy(), A.T.tocsr())
    S = A.copy()
    S.sort_indices()
    assert_same_bits(Td.transpose().to_scipy(), S)


def device_scale(ml, torch, A, d, reverse):
    from mlamg._lib import call, ptr, stream_ptr
    Ad = upload(ml, A)
    dd = torch.as_tensor(np.ascontiguousarray(d, dtype=np.float64)).cuda()
    h = ctypes.c_void_p()
    call("mlamg_csr_scale_rows", Ad.handle, ptr(dd), reverse, ctypes.byref(h), stream_ptr())
    return ml.sparse.DeviceCSR(h).to_scipy()


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", (1, 0))
@pytest.mark.parametrize("name", sorted(SCALE_CASES))
def test_scale_rows(ml, torch_cuda, name, reverse):
    """reverse=1: (diags(d) @ A).tocsr(), zero products dropped (stored zeros, d_i = 0 with
    0 * negative = -0.0, underflow), reversed stored order. reverse=0: A's pattern and order
    with data * d, nothing dropped, -0.0 kept."""
    A, d = scale_case(name)
    assert_same_bits(device_scale(ml, torch_cuda, A, d, reverse), scale_ref(A, d, reverse))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SA_CASES))
def test_sa_smoother(ml, name):
    """I - omega D^-1 A in scipy's order (A's stored order without the diagonal, then the
    diagonal), zeros dropped: the diagonal itself at omega = 1 on power-of-two diagonals."""
    from mlamg._lib import call, stream_ptr
    A, omega, ref = sa_case(name)
    Ad = upload(ml, A)
    h = ctypes.c_void_p()
    call("mlamg_sa_smoother", Ad.handle, float(omega), ctypes.byref(h), stream_ptr())
    assert_same_bits(ml.sparse.DeviceCSR(h).to_scipy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_strength_maps(ml, mode):
    """|a|, 1/|a| (inf for both zeros and for denormals) and 1 on A's own pattern."""
    from mlamg._lib import call, stream_ptr
    A = strength_input()
    assert np.any(A.data < 0) and np.any((A.data == 0.0) & np.signbit(A.data))
    assert np.any(np.abs(A.data) == DENORMAL)
    with np.errstate(divide="ignore", over="ignore"):
        vals = (np.abs(A.data), 1.0 / np.abs(A.data), np.ones(A.nnz))[mode]
    ref = sp.csr_matrix((vals, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    Ad = upload(ml, A)
    h = ctypes.c_void_p()
    call("mlamg_strength", Ad.handle, mode, ctypes.byref(h), stream_ptr())
    assert_same_bits(ml.sparse.DeviceCSR(h).to_scipy(), ref)
