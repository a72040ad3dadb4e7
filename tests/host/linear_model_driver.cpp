// Host model of mlamg_gnn_linear / mlamg_gnn_linear_wide for tests/test_gpu_gnn_wide.py: every
// output is the std::fmaf chain over k = 0 .. K-1 from +0.0 followed by k_linear's epilogue,
//   a = acc (+ b[n]); y = beta != 0 ? beta * Y[m][n] + a : a; relu; (+ R[m][n or 0]).
// Build with -ffp-contract=off (the epilogue's multiply and add round separately, like the
// kernels'). Input file argv[1]:
//   int64 M, K, N, act, has_b, rc | float beta | X[M*K] | W[N*K] | b[N] if has_b |
//   R[M*rc] if rc | Y0[M*N] if beta != 0
// Output file argv[2]: Y[M*N] (float32).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

static bool read_f(FILE* f, std::vector<float>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(float), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t h[6];
  float beta;
  if (std::fread(h, sizeof(int64_t), 6, f) != 6 || std::fread(&beta, sizeof(float), 1, f) != 1)
    return 2;
  const int64_t M = h[0], K = h[1], N = h[2], act = h[3], has_b = h[4], rc = h[5];
  std::vector<float> X, W, b, R, Y;
  if (!read_f(f, X, (size_t)(M * K)) || !read_f(f, W, (size_t)(N * K)) ||
      !read_f(f, b, has_b ? (size_t)N : 0) || !read_f(f, R, (size_t)(M * rc)) ||
      !read_f(f, Y, beta != 0.0f ? (size_t)(M * N) : 0))
    return 2;
  std::fclose(f);
  Y.resize((size_t)(M * N));
  for (int64_t m = 0; m < M; ++m)
    for (int64_t n = 0; n < N; ++n) {
      float acc = 0.0f;
      for (int64_t k = 0; k < K; ++k) acc = std::fmaf(X[m * K + k], W[n * K + k], acc);
      if (has_b) acc = acc + b[n];
      float y = beta != 0.0f ? beta * Y[m * N + n] + acc : acc;
      if (act == 1) y = std::fmax(y, 0.0f);
      if (rc) y = y + R[m * rc + (rc == 1 ? 0 : n)];
      Y[m * N + n] = y;
    }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  if (!Y.empty() && std::fwrite(Y.data(), sizeof(float), Y.size(), o) != Y.size()) return 2;
  std::fclose(o);
  return 0;
}
