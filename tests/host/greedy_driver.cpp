// Host driver of csrc/greedy.cpp for tests/test_greedy_host.py: reads one problem
//   int64 n, nnz | double theta | int32 indptr[n+1] | int32 indices[nnz] | double data[nnz]
// from argv[1], calls mlamg_greedy_coarsening (argv[2] == "null": with F = NULL) and prints
//   rc=<code> nF=<count> nC=<count> untouched=<0|1>
//   F ...
//   C ...
// `untouched`: the outputs still hold the sentinels they were filled with. Built plainly and
// with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "greedy.hpp"

namespace mlamg {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace mlamg

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t head[2];
  double theta;
  if (std::fread(head, sizeof(int64_t), 2, f) != 2 || std::fread(&theta, sizeof(double), 1, f) != 1)
    return 2;
  const int64_t n = head[0], nnz = head[1];
  std::vector<int32_t> ip, ij;
  std::vector<double> a;
  if (!read_n(f, ip, (size_t)(n < 0 ? 0 : n) + 1) || !read_n(f, ij, (size_t)nnz) ||
      !read_n(f, a, (size_t)nnz))
    return 2;
  std::fclose(f);
  const bool null_f = argc > 2 && std::strcmp(argv[2], "null") == 0;
  const int32_t kSentinel = -7;
  std::vector<int32_t> F((size_t)(n < 0 ? 0 : n) + 1, kSentinel), C(F.size(), kSentinel);
  int64_t nF = kSentinel, nC = kSentinel;
  const int rc = mlamg_greedy_coarsening(n, ip.data(), ij.data(), a.data(), theta,
                                         null_f ? nullptr : F.data(), C.data(), &nF, &nC);
  bool untouched = nF == kSentinel && nC == kSentinel;
  for (int32_t v : F) untouched = untouched && v == kSentinel;
  for (int32_t v : C) untouched = untouched && v == kSentinel;
  std::printf("rc=%d nF=%lld nC=%lld untouched=%d\n", rc, (long long)nF, (long long)nC,
              (int)untouched);
  if (rc != MLAMG_OK) {
    std::printf("error %s\n", mlamg::g_err.c_str());
    return 0;
  }
  if (F.back() != kSentinel || C.back() != kSentinel) return 3;  // wrote past n entries
  std::printf("F");
  for (int64_t t = 0; t < nF; ++t) std::printf(" %d", F[t]);
  std::printf("\nC");
  for (int64_t t = 0; t < nC; ++t) std::printf(" %d", C[t]);
  std::printf("\n");
  return 0;
}
