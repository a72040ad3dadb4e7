// Greedy C/F splitting (ns/lib/greedy.py:13-36) on host CSR arrays. The reference keeps U as a
// sorted array and rebuilds it with setdiff1d after every move (O(n^2)); here U is an ordered set
// keyed on (dominance, index), whose first element is np.argmin over the sorted U: the smallest
// dominance, the smallest index among equals. Plain C++: tests/test_greedy_host.py checks it
// against the reference's own results without a device.
#include "greedy.hpp"

#include <cmath>
#include <set>
#include <utility>

namespace mlamg {

namespace {
enum : uint8_t { kU = 0, kF = 1, kC = 2 };
}

void greedy_split(int64_t n, const int32_t* ip, const int32_t* ij, const double* a, double theta,
                  std::vector<int32_t>& F, std::vector<int32_t>& C) {
  F.clear();
  C.clear();
  std::vector<uint8_t> state((size_t)n, kU);
  std::vector<double> dom((size_t)n), diag((size_t)n);
  std::set<std::pair<double, int32_t>> U;
  for (int64_t i = 0; i < n; ++i) {
    double s = 0.0;
    for (int32_t q = ip[i]; q < ip[i + 1]; ++q) {
      s += std::fabs(a[q]);
      if (ij[q] == i) diag[i] = std::fabs(a[q]);
    }
    dom[i] = diag[i] / s;
    if (dom[i] >= theta) {
      state[i] = kF;
      F.push_back((int32_t)i);
    } else {
      U.emplace(dom[i], (int32_t)i);
    }
  }
  while (!U.empty()) {
    const int32_t c = U.begin()->second;
    U.erase(U.begin());
    state[c] = kC;
    C.push_back(c);
    // row c's nonzero columns still in U, ascending (the rows are canonical)
    for (int32_t q = ip[c]; q < ip[c + 1]; ++q) {
      const int32_t i = ij[q];
      if (a[q] == 0.0 || state[i] != kU) continue;
      double su = 0.0, sf = 0.0;  // over U and over F as they stand now; C drops out
      for (int32_t t = ip[i]; t < ip[i + 1]; ++t) {
        const uint8_t st = state[ij[t]];
        if (st == kU) su += std::fabs(a[t]);
        else if (st == kF) sf += std::fabs(a[t]);
      }
      U.erase(std::make_pair(dom[i], i));
      dom[i] = diag[i] / (su + sf);
      if (dom[i] >= theta) {
        state[i] = kF;
        F.push_back(i);
      } else {
        U.emplace(dom[i], i);
      }
    }
  }
}

}  // namespace mlamg

extern "C" int mlamg_greedy_coarsening(int64_t n, const int32_t* indptr, const int32_t* indices,
                                       const double* data, double theta, int32_t* F, int32_t* C,
                                       int64_t* nF, int64_t* nC) {
  auto fail = [](const char* msg) {
    mlamg::set_error(std::string("mlamg_greedy_coarsening: ") + msg);
    return MLAMG_EINVAL;
  };
  if (n < 0 || n >= INT32_MAX) return fail("n out of range");
  if (!indptr || !nF || !nC) return fail("NULL argument");
  if (n > 0 && (!F || !C)) return fail("NULL argument");
  if (std::isnan(theta)) return fail("theta is NaN");
  if (indptr[0] != 0) return fail("indptr must start at 0");
  for (int64_t i = 0; i < n; ++i)
    if (indptr[i + 1] < indptr[i]) return fail("indptr decreases");
  if (indptr[n] > 0 && (!indices || !data)) return fail("NULL argument");
  for (int64_t i = 0; i < n; ++i) {
    bool has_diag = false;
    for (int32_t q = indptr[i]; q < indptr[i + 1]; ++q) {
      const int32_t j = indices[q];
      if (j < 0 || j >= n) return fail("column index out of range");
      if (q > indptr[i] && indices[q - 1] >= j) return fail("rows must be canonical (ascending, "
                                                             "duplicate-free columns)");
      if (!std::isfinite(data[q])) return fail("non-finite value");
      if (j == i) {
        if (data[q] == 0.0) return fail("zero diagonal");
        has_diag = true;
      }
    }
    if (!has_diag) return fail("missing diagonal");
  }
  std::vector<int32_t> f, c;
  mlamg::greedy_split(n, indptr, indices, data, theta, f, c);
  for (size_t t = 0; t < f.size(); ++t) F[t] = f[t];
  for (size_t t = 0; t < c.size(); ++t) C[t] = c[t];
  *nF = (int64_t)f.size();
  *nC = (int64_t)c.size();
  return MLAMG_OK;
}
