"""pyamg.relaxation (4.x) subset."""
from . import chebyshev, relaxation  # noqa: F401
