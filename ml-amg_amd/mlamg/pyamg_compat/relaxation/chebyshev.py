"""pyamg.relaxation.chebyshev (4.x): the coefficients of the polynomial smoother. Host only
(numpy); pyamg is absent, the function is restated from pyamg 4.x."""
import numpy as np


def chebyshev_polynomial_coefficients(a, b, degree):
    """Coefficients (highest power first, degree + 1 numbers, the last one 1) of the Chebyshev
    polynomial of the given degree that is smallest on [a, b] among those with p(0) = 1: its
    roots are the Chebyshev points of [a, b]. 0 < a < b, else ValueError."""
    if a >= b or a <= 0:
        raise ValueError(f'invalid interval [{a},{b}]')
    # Chebyshev roots for the interval [-1, 1]
    std_roots = np.cos(np.pi * (np.arange(degree) + 0.5) / degree)
    # Chebyshev roots for the interval [a, b]
    scaled_roots = 0.5 * (b - a) * (1 + std_roots) + a
    # the monic polynomial with these roots, scaled so that p(0) = 1
    scaled_poly = np.poly(scaled_roots)
    scaled_poly /= np.polyval(scaled_poly, 0)
    return scaled_poly
