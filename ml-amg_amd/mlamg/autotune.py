"""SpMV format autotune: the candidate tables, the byte lower bound, the timed launch, the search
over one operator's candidates and the cache of its decisions.

Every candidate of a family computes the same bits, so the search is a timing decision only: host
arithmetic over two callbacks (time a format; did the value dictionary apply). The module imports
without torch and without the native library; only time_format touches the device. Callers:
Hierarchy.apply_formats and distributed.tune_local, each passing the rules that hold there.
"""
import statistics

EXACT_CANDIDATES = (("csr_stream", 0), ("sell", 1), ("sell", 512), ("sorted", 0),
                    ("sorted", 2), ("sell_dict", 1), ("sell_dict", 512), ("rowpat", 0))
LONG_CANDIDATES = (("long", 0),)
VECTOR_CANDIDATES = (("vector", 64), ("vector", 128), ("vector", 256), ("vector", 512))

# bytes read between two timed launches of the autotune, so each one starts with the
# operator and x out of the caches (L2 4 MB per XCD, MALL 256 MB) as in the cycle, where the
# other levels' streams pass in between; a read leaves no dirty lines to write back during
# the timed launch
FLUSH_BYTES = 512 << 20

# Autotune pruning: the fewest bytes per stored nonzero a format can stream (sorted: 4-byte
# packed index + a 1-byte value code when the values fit a dictionary; sell_dict: a 2-byte
# code; rowpat: ~0, one byte per pair of rows; vector: 16-bit indices) at 7 TB/s: no
# candidate can beat that from a cold cache (the autotune reads 512 MB, twice the MALL,
# before each timed launch; 8 TB/s is the HBM peak, ~6.3 TB/s what streams reach, and the
# fastest cold kernel measured here runs at 3.7 TB/s of its bytes). A pruned candidate costs
# nothing but a timing chance: every format of the family computes the same bits. (Round 4:
# 8 -> 7 TB/s, so that e.g. SELL and CSR-stream are no longer built and timed for P_0 / R_0,
# whose sorted format already beats their bytes at 7 TB/s.)
FORMAT_MIN_BYTES_PER_NNZ = {"csr_stream": 12.0, "sell": 12.0, "sorted": 5.0, "sell_dict": 2.0,
                            "rowpat": 0.0, "long": 12.0, "vector": 10.0}
LB_PEAK_BPS = 7e12
# a SELL / dictionary-SELL timed at more than this many times the best format so far skips
# its sigma-sorted (row-length-ordered) variant
SIGMA_SKIP_RATIO = 1.5

UNSUPPORTED = -5  # _lib.MLAMG_EUNSUPPORTED: the operator does not allow the format


def lower_bound_us(M, kind, fmt):
    """Time (us) of M's cycle operation (kind 'A', 'P' or 'R', see time_format) in format fmt at
    LB_PEAK_BPS for the fewest bytes the format can stream."""
    n_rows, n_cols = M.shape
    vec = 8.0 * (n_cols + n_rows + (n_rows if kind in ("A", "P") else 0))  # x, y (+ b / y in)
    return (FORMAT_MIN_BYTES_PER_NNZ[fmt] * M.nnz + vec) / LB_PEAK_BPS * 1e6


def candidates_for(M, family):
    """The candidates of M in its family: 'vector' the four CSR-vector widths, 'exact' the
    scipy-order formats, with the long-row tiles from a mean row of 16 entries."""
    if family == "vector":
        return list(VECTOR_CANDIDATES)
    cands = list(EXACT_CANDIDATES)
    if M.nnz >= 16 * max(M.shape[0], 1):
        cands += list(LONG_CANDIDATES)
    return cands


def time_format(M, fmt, arg, x, y, reps=5, kind="A", flush=None):
    """Median time of M's cycle operation in format fmt over `reps` launches, each after a
    cache flush (a read of `flush`): the residual epilogue for A (r = b - A x, as in the
    cycle; here b = y), y += M x for P, y = M x for R. Timing a launch repeated back to back
    measures cache-resident operators (any operator up to the MALL's size), which
    favoured formats that are not the fastest in the cycle."""
    import torch

    from ._lib import call, ptr, stream_ptr
    M.set_format(fmt, arg)
    if kind == "A":
        def op():
            call("mlamg_residual", M.handle, ptr(y), ptr(x), ptr(y), None, stream_ptr())
    elif kind == "P":
        def op():
            call("mlamg_prolong_add", M.handle, ptr(x), ptr(y), stream_ptr())
    else:
        def op():
            M.matvec(x, out=y)
    op()
    s = torch.cuda.current_stream()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(reps)]
    sink = torch.empty((), dtype=flush.dtype, device=flush.device) if flush is not None else None
    for e0, e1 in ev:
        if flush is not None:
            torch.sum(flush, dim=0, out=sink)
        e0.record(s)
        op()
        e1.record(s)
    ev[-1][1].synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3  # us


def search(cands, lbs, time_one, *, refuses_family, first=None, sigma_skip=None,
           value_dict=None):
    """Time one operator's candidates (fmt, arg): (chosen 'fmt/arg', {name: us} of those timed,
    names of those neither built nor timed). time_one(fmt, arg) builds and times one, or raises
    an error whose `code` is UNSUPPORTED (any other propagates). `first`, then the most compact
    formats (lbs: lower_bound_us per candidate) first; a candidate whose bytes could not move
    in less than the best time so far, even at LB_PEAK_BPS, is pruned. The call site's rules:
      refuses_family(fmt, arg)  whether a refused build prunes the format's other variants;
      sigma_skip  a SELL / dictionary SELL (arg 1) timed at more than this many times the best
                  so far prunes its sigma-sorted variant (None: no such rule);
      value_dict  asked once sorted/0 is timed; true (the <= 256-value table applied) prunes
                  sorted/2, whose block dictionaries would be refused (None: no such rule)."""
    times, pruned, refused = {}, [], set()
    has_value_dict = False
    for fmt, arg in sorted(cands, key=lambda c: (c != first, lbs[c])):
        if (times and lbs[(fmt, arg)] >= min(times.values())) or fmt in refused \
                or ((fmt, arg) == ("sorted", 2) and has_value_dict):
            pruned.append(f"{fmt}/{arg}")
            continue
        try:
            t = time_one(fmt, arg)
        except Exception as e:  # format limits (e.g. sorted: row > 4096 nnz)
            if getattr(e, "code", None) != UNSUPPORTED:
                raise
            if refuses_family(fmt, arg):
                refused.add(fmt)
            continue
        times[f"{fmt}/{arg}"] = t
        if value_dict is not None and (fmt, arg) == ("sorted", 0):
            has_value_dict = bool(value_dict())
        if sigma_skip is not None and fmt in ("sell", "sell_dict") and arg == 1 \
                and t > sigma_skip * min(times.values()):
            refused.add(fmt)
    return (min(times, key=times.get), {k: round(v, 2) for k, v in times.items()}, pruned)


# Decisions per operator signature (kind, shape, nnz, fingerprint of rows, columns and value
# bits, candidate family): a hierarchy rebuilt on the same operator (a dataset loop re-solving
# one grid, a distributed rank rebuilding rank 0's hierarchy) takes the same kernel without
# re-timing (VERDICT r04 Next #7). The choice is a timing decision only — every candidate of a
# family computes the same bits — so a stale entry costs speed, never a result. Bounded, first
# in first out; emptied by clear().
TUNE_CACHE_MAX = 256
_cache = {}


def cached(key, run):
    """The record of `key`: the stored one with cached=True added, else run()'s (a search),
    stored; at TUNE_CACHE_MAX entries the oldest leaves."""
    hit = _cache.get(key)
    if hit is not None:
        return dict(hit, cached=True)
    record = run()
    if len(_cache) >= TUNE_CACHE_MAX:
        _cache.pop(next(iter(_cache)))
    _cache[key] = record
    return record


def clear():
    _cache.clear()
