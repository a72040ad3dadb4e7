// Stand-alone driver of the batched solver's host planner (csrc/batch_plan.cpp): no GPU, no HIP.
// Reads problems from a text file (or stdin), plans them `passes` times and prints what the
// planner decided, for tests/test_batch_plan_host.py to compare with its numpy restatement.
//
// Input (whitespace-separated):
//   passes smoother nu_pre nu_post max_iter count
//   then per problem: n n_c A_nnz P_nnz, A.indptr, A.indices, A.data, P.indptr, P.indices, P.data
// Output per pass: a "plan" line, then per problem a "prob" line of key=value fields and the
// level pointers ("lev") and level-order rows ("pkr0") as the kernels would read them from the
// arena's host copy.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "batch_plan.hpp"

namespace {

struct Csr {
  std::vector<int32_t> indptr, indices;
  std::vector<double> data;
  void read(std::istream& in, int64_t rows, int64_t nnz) {
    indptr.resize(rows + 1);
    indices.resize(nnz);
    data.resize(nnz);
    for (auto& v : indptr) in >> v;
    for (auto& v : indices) in >> v;
    for (auto& v : data) in >> v;
  }
};

struct Problem {
  Csr A, P;
  std::vector<double> b, x0, x, err;
};

void print_ints(const char* name, int q, const char* buf, int64_t off, int64_t cnt) {
  const int32_t* v = reinterpret_cast<const int32_t*>(buf + off);
  std::printf("%s %d:", name, q);
  for (int64_t i = 0; i < cnt; ++i) std::printf(" %d", v[i]);
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  std::ifstream file;
  if (argc > 1) file.open(argv[1]);
  std::istream& in = argc > 1 ? static_cast<std::istream&>(file) : std::cin;
  int passes, smoother, nu_pre, nu_post, max_iter, count;
  in >> passes >> smoother >> nu_pre >> nu_post >> max_iter >> count;
  if (!in || count < 1) return std::fprintf(stderr, "bad header\n"), 2;
  std::vector<Problem> store(count);
  std::vector<mlamg_amg2v_problem> probs(count);
  for (int q = 0; q < count; ++q) {
    mlamg_amg2v_problem& p = probs[q];
    Problem& s = store[q];
    p = mlamg_amg2v_problem{};
    in >> p.n >> p.n_c >> p.A_nnz >> p.P_nnz;
    if (!in || p.n < 0 || p.A_nnz < 0 || p.P_nnz < 0) return std::fprintf(stderr, "bad sizes\n"), 2;
    s.A.read(in, p.n, p.A_nnz);
    s.P.read(in, p.n, p.P_nnz);
    if (!in) return std::fprintf(stderr, "short input\n"), 2;
    s.b.assign(p.n, 1.0);
    s.x0.assign(p.n, 0.0);
    s.x.assign(p.n, 0.0);
    s.err.assign(max_iter > 0 ? max_iter : 1, 0.0);
    p.A_indptr = s.A.indptr.data(), p.A_indices = s.A.indices.data(), p.A_data = s.A.data.data();
    p.P_indptr = s.P.indptr.data(), p.P_indices = s.P.indices.data(), p.P_data = s.P.data.data();
    p.b = s.b.data(), p.x0 = s.x0.data(), p.x_out = s.x.data(), p.err_out = s.err.data();
  }
  for (int pass = 0; pass < passes; ++pass) {
    mlamg::BatchPlan plan;
    const int rc = mlamg::plan_batch(probs.data(), count, smoother, nu_pre, nu_post, 1.0, 0, 1e-10,
                                     max_iter, &plan);
    std::printf("plan pass=%d code=%d phased=%d r_lds=%d any_band=%d ext_coarse=%d batch_ext=%d "
                "two_pass=%d rp=%d err=%s\n",
                pass, rc, plan.phased, plan.r_lds, plan.any_band, plan.ext_coarse, plan.batch_ext,
                plan.two_pass, plan.rp, plan.err.c_str());
    if (rc != MLAMG_OK) continue;
    std::vector<char> buf(plan.in_bytes);
    mlamg::fill_inputs(plan, probs.data(), buf.data());
    for (int q = 0; q < count; ++q) {
      const mlamg::BDesc& D = plan.desc[q];
      std::printf("prob %d spd=%d band_ld=%d nlev=%d K=%d KA=%d KP=%d KT=%d panel=%d chol_nb=%d "
                  "gs_rw=%d gs_db=%d gs_rp=%d n_chunks=%d cap=%d setup_mode=%d phased=%d "
                  "ak_col=%lld pk_row0=%lld a_raw=%lld b=%lld\n",
                  q, D.spd, D.band_ld, D.nlev, D.K, D.KA, D.KP, D.KT, D.panel, D.chol_nb, D.gs_rw,
                  D.gs_db, D.gs_rp, D.n_chunks, D.cap, D.setup_mode, D.phased,
                  (long long)D.ak_col, (long long)D.pk_row0, (long long)D.a_raw, (long long)D.b);
      if (smoother != 0) continue;
      print_ints("lev", q, buf.data(), D.lev_ptr, D.nlev + 1);
      print_ints("pkr0", q, buf.data(), D.pk_row0, D.n);
    }
  }
  return 0;
}
