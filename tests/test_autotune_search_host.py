"""CPU, no native library: the format search of mlamg.autotune, driven by scripted timings on
fake operators — the candidate order, the byte-bound pruning, the refusal bookkeeping, the rules
of its two call sites (Hierarchy.apply_formats, distributed.tune_local) and the cache."""
import sys

import pytest

from mlamg import autotune
from mlamg.autotune import candidates_for, lower_bound_us, search


class _Op:
    def __init__(self, n, nnz):
        self.shape = (n, n)
        self.nnz = nnz


class _Refused(RuntimeError):
    def __init__(self, code=autotune.UNSUPPORTED):
        super().__init__(f"refused ({code})")
        self.code = code


C4_A0 = _Op(10077696, 70263936)
SMALL = _Op(1000, 7000)
C4_ORDER = ["rowpat/0", "sell_dict/1", "sell_dict/512", "sorted/0", "sorted/2", "csr_stream/0",
            "sell/1", "sell/512"]
SMALL_US = {"rowpat/0": 10, "sell_dict/1": 16, "sorted/0": 12, "sorted/2": 11, "csr_stream/0": 9,
            "sell/1": 14}


def _script(script):
    """time_one over a dict 'fmt/arg' -> microseconds or an exception to raise; a candidate the
    script does not name must not be timed. Returns (time_one, the names timed or tried)."""
    seen = []

    def time_one(fmt, arg):
        name = f"{fmt}/{arg}"
        seen.append(name)
        assert name in script, f"{name} must not be built"
        if isinstance(script[name], Exception):
            raise script[name]
        return script[name]
    return time_one, seen


def _as_apply_formats(M, script, value_dict=False, kind="A"):
    """The rule set Hierarchy.apply_formats passes."""
    cands = candidates_for(M, "exact")
    time_one, seen = _script(script)
    out = search(cands, {c: lower_bound_us(M, kind, c[0]) for c in cands}, time_one,
                 refuses_family=lambda fmt, arg: (fmt in ("sell_dict", "sell")
                                                  or (fmt, arg) == ("sorted", 0)),
                 sigma_skip=autotune.SIGMA_SKIP_RATIO, value_dict=lambda: value_dict)
    return out, seen


def _as_tune_local(M, script, first, kind="A"):
    """The rule set distributed.tune_local passes."""
    cands = candidates_for(M, "exact")
    time_one, seen = _script(script)
    out = search(cands, {c: lower_bound_us(M, kind, c[0]) for c in cands}, time_one,
                 first=first, refuses_family=lambda fmt, arg: True)
    return out, seen


def test_module_needs_neither_torch_nor_the_library():
    import subprocess
    code = ("import sys; import mlamg.autotune; "
            "assert 'torch' not in sys.modules and 'mlamg._lib' not in sys.modules")
    env_path = [p for p in sys.path if p]
    subprocess.run([sys.executable, "-c", f"import sys; sys.path[:0] = {env_path!r}; {code}"],
                   check=True)


def test_unsupported_code_is_the_library_s():
    """UNSUPPORTED restates include/mlamg.h's MLAMG_EUNSUPPORTED."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mlamg.h")) as f:
        m = re.search(r"#define MLAMG_EUNSUPPORTED (-?\d+)", f.read())
    assert m and int(m.group(1)) == autotune.UNSUPPORTED


def test_c4_fine_operator_order_bounds_and_pruning():
    cands = candidates_for(C4_A0, "exact")
    assert ("long", 0) not in cands  # nnz < 16 n
    lbs = {f"{f}/{a}": lower_bound_us(C4_A0, "A", f) for f, a in cands}
    for names, bound in ((C4_ORDER[:1], 34.55), (C4_ORDER[1:3], 54.63), (C4_ORDER[3:5], 84.74),
                         (C4_ORDER[5:], 155.0)):
        for name in names:
            assert lbs[name] == pytest.approx(bound, abs=0.006), name
    (chosen, us, pruned), seen = _as_apply_formats(C4_A0, {"rowpat/0": 44.6})
    assert seen == ["rowpat/0"]
    assert chosen == "rowpat/0" and us == {"rowpat/0": 44.6}
    assert pruned == C4_ORDER[1:]


def test_c4_fine_operator_with_rowpat_refused():
    (chosen, us, pruned), seen = _as_apply_formats(
        C4_A0, {"rowpat/0": _Refused(), "sell_dict/1": 95, "sell_dict/512": 90, "sorted/0": 100},
        value_dict=True)
    assert seen == ["rowpat/0", "sell_dict/1", "sell_dict/512", "sorted/0"]
    assert chosen == "sell_dict/512"
    assert us == {"sell_dict/1": 95, "sell_dict/512": 90, "sorted/0": 100}
    assert pruned == ["sorted/2", "csr_stream/0", "sell/1", "sell/512"]


def test_sigma_skip():
    (chosen, us, pruned), seen = _as_apply_formats(SMALL, SMALL_US)
    assert chosen == "csr_stream/0"
    assert pruned == ["sell_dict/512", "sell/512"]  # 16 > 1.5 * 10 and 14 > 1.5 * 9
    assert seen == ["rowpat/0", "sell_dict/1", "sorted/0", "sorted/2", "csr_stream/0", "sell/1"]
    assert us == SMALL_US


def test_value_dictionary_prunes_the_block_dictionaries():
    script = {k: v for k, v in SMALL_US.items() if k != "sorted/2"}
    (chosen, _, pruned), _ = _as_apply_formats(SMALL, script, value_dict=True)
    assert chosen == "csr_stream/0"
    assert pruned == ["sell_dict/512", "sorted/2", "sell/512"]


def test_refusal_propagation():
    script = dict(SMALL_US, **{"sell_dict/1": _Refused(), "sorted/0": _Refused()})
    del script["sorted/2"]  # sorted/2 and sell_dict/512 must not be built
    (chosen, us, pruned), seen = _as_apply_formats(SMALL, script)
    assert "sell_dict/512" in pruned and "sorted/2" in pruned
    assert "sell_dict/1" not in pruned and "sell_dict/1" not in us
    assert chosen == "csr_stream/0"
    # a refused rowpat, csr_stream or sorted/2 refuses nothing else
    script = dict(SMALL_US, **{"rowpat/0": _Refused(), "sorted/2": _Refused(),
                               "csr_stream/0": _Refused(), "sell_dict/512": 15,
                               "sell/512": 13})
    (chosen, us, pruned), _ = _as_apply_formats(SMALL, script)
    assert chosen == "sorted/0" and pruned == []
    assert us == {"sell_dict/1": 16, "sell_dict/512": 15, "sorted/0": 12, "sell/1": 14,
                  "sell/512": 13}
    # any other error propagates
    for err in (_Refused(code=-2), ValueError("no code")):
        with pytest.raises(type(err)):
            _as_apply_formats(SMALL, dict(SMALL_US, **{"sorted/0": err}))


def test_tune_local_rules():
    script = dict(SMALL_US, **{"sell_dict/512": 15, "sell/512": 13})
    (chosen, us, pruned), seen = _as_tune_local(SMALL, script, first=("sorted", 0))
    # the global choice first, then the rest by bound; no sigma rule, no value-dictionary rule
    assert seen == ["sorted/0", "rowpat/0", "sell_dict/1", "sell_dict/512", "sorted/2",
                    "csr_stream/0", "sell/1", "sell/512"]
    assert chosen == "csr_stream/0" and pruned == [] and us == script
    # every refused build refuses its family; other families are left alone
    script = dict(script, **{"rowpat/0": _Refused(), "sell/1": _Refused()})
    del script["sell/512"]
    (chosen, us, pruned), seen = _as_tune_local(SMALL, script, first=("sorted", 0))
    assert chosen == "csr_stream/0" and pruned == ["sell/512"]
    assert seen == ["sorted/0", "rowpat/0", "sell_dict/1", "sell_dict/512", "sorted/2",
                    "csr_stream/0", "sell/1"]
    with pytest.raises(_Refused):
        _as_tune_local(SMALL, dict(script, **{"sorted/2": _Refused(code=-1)}), ("sorted", 0))


def test_candidates_for():
    n = 1000
    assert ("long", 0) not in candidates_for(_Op(n, 16 * n - 1), "exact")
    for nnz in (16 * n, 16 * n + 1):
        cands = candidates_for(_Op(n, nnz), "exact")
        assert cands[-1] == ("long", 0) and cands[:-1] == list(autotune.EXACT_CANDIDATES)
    assert candidates_for(_Op(n, 400 * n), "vector") == [("vector", w)
                                                         for w in (64, 128, 256, 512)]


def test_cache():
    autotune.clear()
    calls = []

    def run(tag):
        def go():
            calls.append(tag)
            return {"chosen": "rowpat/0", "us": {"rowpat/0": float(tag)}, "pruned": []}
        return go
    first = autotune.cached("k0", run(0))
    assert first == {"chosen": "rowpat/0", "us": {"rowpat/0": 0.0}, "pruned": []}
    hit = autotune.cached("k0", run(99))
    assert hit == dict(first, cached=True) and calls == [0]  # a hit times nothing
    assert "cached" not in first
    assert autotune.TUNE_CACHE_MAX == 256
    for i in range(1, 256):
        autotune.cached(f"k{i}", run(i))
    assert autotune.cached("k0", run(99))["cached"] and len(calls) == 256
    autotune.cached("k256", run(256))  # entry 257 evicts the oldest, k0
    assert "cached" not in autotune.cached("k0", run(1000)) and calls[-1] == 1000
    assert autotune.cached("k256", run(99)).get("cached") and calls[-1] == 1000
    autotune.clear()
    assert "cached" not in autotune.cached("k256", run(7)) and calls[-1] == 7
    autotune.clear()
