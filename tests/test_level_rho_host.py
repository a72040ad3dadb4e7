"""CPU: pyamg_setup.level_rho, the per-level spectral-radius rule of Hierarchy.pyamg_sa (rho)
and of the Chebyshev smoother (smoother_rho). Host arithmetic; no device call is made."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ml-amg_amd", "mlamg", "libmlamg_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libmlamg_hip.so not built")


def test_level_rho():
    from mlamg.pyamg_setup import level_rho
    none = {}
    # a number applies to every level
    assert [level_rho(1.75, lvl, none) for lvl in range(3)] == [1.75] * 3
    assert isinstance(level_rho(2, 1, none), float)
    # a list (or tuple) gives its entry per level
    assert [level_rho([1.5, 2.5, 3.5], lvl, none) for lvl in range(3)] == [1.5, 2.5, 3.5]
    assert level_rho((1.5, 2.5), 1, none) == 2.5
    # a short list raises, naming the argument and the level
    with pytest.raises(ValueError, match="^no rho given for level 2$"):
        level_rho([1.5, 2.5], 2, none)
    with pytest.raises(ValueError, match="^no smoother_rho given for level 1$"):
        level_rho([1.5], 1, none, "smoother_rho")
    with pytest.raises(ValueError, match="^no rho given for level 0$"):
        level_rho(None, 0, none)
    # a named estimate is computed for the level, and only when asked for
    calls = []
    est = {"arnoldi": lambda: calls.append("a") or 7.0, "lanczos": lambda: calls.append("l") or 9.0}
    assert level_rho("arnoldi", 0, est) == 7.0 and calls == ["a"]
    assert level_rho(3.0, 0, est) == 3.0 and calls == ["a"]
    # a name the call site does not offer is no number
    with pytest.raises(ValueError):
        level_rho("lanczos", 0, {"arnoldi": est["arnoldi"]})
