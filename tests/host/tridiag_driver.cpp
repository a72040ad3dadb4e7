// Stand-alone driver of the Lanczos driver's bisection (csrc/tridiag.hpp): no GPU, no HIP. For
// every tridiagonal of IN it writes the largest eigenvalue and the Sturm counts at the query
// points, for tests/test_tridiag_host.py to compare with LAPACK.
//
// Usage: tridiag_driver IN OUT
//   IN  (binary): int32 count, then per matrix int32 m, int32 nq, float64 a[m], float64 b[m]
//                 (b[0] is not read by the routines; b[i] couples rows i - 1 and i), float64 x[nq]
//   OUT (binary): per matrix float64 tridiag_max_eig, then float64 sturm_count(x[k]) for each k
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tridiag.hpp"

namespace {

template <class T>
bool read(std::FILE* f, std::vector<T>& v, size_t count) {
  v.resize(count);
  return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return std::fprintf(stderr, "usage: tridiag_driver IN OUT\n"), 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return std::fprintf(stderr, "cannot open files\n"), 2;
  std::vector<int32_t> head;
  if (!read(in, head, 1) || head[0] < 0) return std::fprintf(stderr, "short input\n"), 2;
  const int count = head[0];
  for (int p = 0; p < count; ++p) {
    std::vector<double> a, b, x;
    if (!read(in, head, 2) || head[0] < 1 || head[1] < 0 || !read(in, a, head[0]) ||
        !read(in, b, head[0]) || !read(in, x, head[1]))
      return std::fprintf(stderr, "short input at matrix %d\n", p), 2;
    const int m = head[0];
    std::vector<double> res;
    res.push_back(mlamg::tridiag_max_eig(a, b, m));
    for (double xk : x) res.push_back((double)mlamg::sturm_count(a, b, m, xk));
    std::fwrite(res.data(), sizeof(double), res.size(), out);
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return std::fprintf(stderr, "write failed\n"), 2;
  std::printf("matrices %d\n", count);
  return 0;
}
