// Stand-alone driver of the Gauss-Seidel host planner (csrc/gs_plan.cpp): no GPU, no HIP. Plans
// one sweep direction of one CSR matrix and writes what the planner decided, for
// tests/test_gs_plan_host.py to compare with its numpy restatement and to check invariants on.
//
// Usage: gs_plan_driver IN OUT
//   IN  (binary): int32 n nnz backward block no_win no_ring no_lds no_wring no_wave wave_lpr,
//                 int32 indptr[n + 1], int32 indices[nnz], float64 data[nnz]
//   OUT (binary): the plan's arrays, back to back
// stdout: one "scalars" line of key=value fields, then per array "array NAME DTYPE COUNT" in the
// order they lie in OUT (DTYPE i4, u2 or f8).
#include <cstdio>
#include <vector>

#include "gs_plan.hpp"

namespace {

template <class T>
bool read(std::FILE* f, std::vector<T>& v, size_t count) {
  v.resize(count);
  return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}

template <class T>
void dump(std::FILE* f, const char* name, const char* dtype, const T* v, size_t count) {
  if (count) std::fwrite(v, sizeof(T), count, f);
  std::printf("array %s %s %zu\n", name, dtype, count);
}

void dump(std::FILE* f, const char* name, const std::vector<int32_t>& v) {
  dump(f, name, "i4", v.data(), v.size());
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return std::fprintf(stderr, "usage: gs_plan_driver IN OUT\n"), 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return std::fprintf(stderr, "cannot open files\n"), 2;
  std::vector<int32_t> head, ip, ij;
  std::vector<double> ax;
  if (!read(in, head, 10) || head[0] < 0 || head[1] < 0 || !read(in, ip, (size_t)head[0] + 1) ||
      !read(in, ij, head[1]) || !read(in, ax, head[1]))
    return std::fprintf(stderr, "short input\n"), 2;
  std::fclose(in);
  mlamg::GsKnobs knobs;
  knobs.no_win = head[4], knobs.no_ring = head[5], knobs.no_lds = head[6];
  knobs.no_wring = head[7], knobs.no_wave = head[8], knobs.wave_lpr = head[9];
  mlamg::GsPlan P;
  mlamg::gs_plan_structure(ip.data(), ij.data(), head[0], head[2] != 0, P);
  mlamg::gs_plan_layouts(ip.data(), ij.data(), P.packed ? ax.data() : nullptr, head[3] != 0,
                         knobs, P);
  std::printf("scalars path=%d n_levels=%d max_level_rows=%d max_off=%d max_len=%d K=%d packed=%d "
              "window=%d ring=%d pipe_lds=%d wring=%d wave=%d wave_lpr=%d wave_epl=%d ring_w=%d "
              "ring_log2_r=%d ring_lds=%zu wr_lpr=%d wr_epl=%d wr_w=%d wr_log2=%d wr_lds=%zu "
              "win_rw=%d win_w=%d win_cap=%d ring_log2=%d n_chunks=%d win_lds=%zu\n",
              (int)P.path, P.n_levels, P.max_level_rows, P.max_off, P.max_len, P.K, P.packed,
              P.window, P.ring, P.pipe_lds, P.wring, P.wave, P.wave_lpr, P.wave_epl, P.ring_w,
              P.ring_log2_r, P.ring_lds, P.wr_lpr, P.wr_epl, P.wr_w, P.wr_log2, P.wr_lds, P.win_rw,
              P.win_w, P.win_cap, P.ring_log2, P.n_chunks, P.win_lds);
  dump(out, "level", P.level);
  dump(out, "level_ptr", P.level_ptr);
  dump(out, "rows", P.rows);
  dump(out, "pcol", P.pcol);
  dump(out, "pval", "f8", P.pval.data(), P.pval.size());
  dump(out, "pdiag", "f8", P.pdiag.data(), P.pdiag.size());
  dump(out, "wpos", P.wpos);
  dump(out, "rcol", P.rcol);
  dump(out, "rcode", "u2", P.rcode.data(), P.rcode.size());
  dump(out, "wr_code", P.wr_code);
  dump(out, "wr_len", P.wr_len);
  dump(out, "wr_st", "i4", reinterpret_cast<const int32_t*>(P.wr_st.data()), 2 * P.wr_st.size());
  dump(out, "wcol", P.wcol);
  dump(out, "clev", P.clev);
  return std::fclose(out) == 0 ? 0 : 2;
}
