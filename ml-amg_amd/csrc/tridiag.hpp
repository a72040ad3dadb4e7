// Largest eigenvalue of a symmetric tridiagonal matrix by bisection on Sturm counts: the host
// half of the Lanczos in eig.hip. Host-only and free of HIP, so that tests/host/tridiag_driver.cpp
// compiles it with g++ (tests/test_tridiag_host.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

namespace mlamg {

// number of eigenvalues of the symmetric tridiagonal (a[0..m), b[1..m)) smaller than x
static int sturm_count(const std::vector<double>& a, const std::vector<double>& b, int m, double x) {
  int cnt = 0;
  double q = 1.0;
  for (int i = 0; i < m; ++i) {
    const double bb = i > 0 ? b[i] * b[i] : 0.0;
    q = (a[i] - x) - (i > 0 ? bb / q : 0.0);
    if (q == 0.0) q = -1e-300;
    if (q < 0.0) ++cnt;
  }
  return cnt;
}

static double tridiag_max_eig(const std::vector<double>& a, const std::vector<double>& b, int m) {
  double lo = a[0], hi = a[0];
  for (int i = 0; i < m; ++i) {
    const double r = (i > 0 ? std::fabs(b[i]) : 0.0) + (i + 1 < m ? std::fabs(b[i + 1]) : 0.0);
    lo = std::min(lo, a[i] - r);
    hi = std::max(hi, a[i] + r);
  }
  for (int it = 0; it < 200; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (mid <= lo || mid >= hi) break;
    if (sturm_count(a, b, m, mid) == m) hi = mid;  // all eigenvalues < mid
    else lo = mid;
  }
  return hi;
}

}  // namespace mlamg
