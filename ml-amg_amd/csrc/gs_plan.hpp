// What the Gauss-Seidel kernels (gs.hip) and their host planner (gs_plan.cpp) must agree on,
// written once: the kernels' limits and slot codes, the level recurrence, and the plan of one
// sweep direction as a host value. Host-only: standard headers, no HIP — the planner builds and
// runs (and is tested, tests/test_gs_plan_host.py) without a GPU toolchain.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define MLAMG_GS_HD __host__ __device__
#else
#define MLAMG_GS_HD
#endif

namespace mlamg {

constexpr int kGsBlock = 1024;                          // one workgroup of the whole-sweep kernels
constexpr int kGsBlockMaxLevelRows = 8 * kGsBlock;      // widest level of k_gs_block / k_gs_wave
constexpr int kGsWaveMaxLPR = 16;  // lanes per row: 8 for rows of <= 64 entries (128 rows per
                                   // pass), 16 up to 128 entries
constexpr int kGsRingK = 4;
constexpr size_t kGsRingLdsMax = 150 * 1024;  // the ring, its sink slot and the level starts
constexpr uint32_t kGsRingPad = 0xFFFF, kGsRingLater = 0xFFFE;  // the 16-bit slot codes
constexpr int32_t kGsWringPad = -1, kGsWringLater = -2, kGsWringDiag = -3, kGsWringFar = -16;
constexpr size_t kGsWringLdsMax = 150 * 1024;
constexpr int kGsRingMaxLog2 = 13;  // ring and long-row ring: at most 8,192 slots
constexpr int kGsLdsMax = 8192;     // 64 KB of x: within the default dynamic-LDS limit
constexpr size_t kGsWinLdsMax = 150 * 1024;  // the window's ring and its two staging buffers

// one staging buffer of cap + 1 positions (the last: the dummy of lanes past a level's end),
// 16-byte aligned sections: vals (cap+1) x KM | diag | b (doubles) | level starts
// (cap + 2 int32) | columns (cap+1) x KM (uint16 ring slots), after a 16-byte header (levels,
// first position, positions)
MLAMG_GS_HD constexpr int64_t win_a16(int64_t b) { return (b + 15) & ~int64_t(15); }
MLAMG_GS_HD constexpr int64_t win_buf_bytes(int64_t cap, int KM) {
  return 16 + win_a16(8 * (cap + 1) * KM) + 2 * win_a16(8 * (cap + 1)) + win_a16(4 * (cap + 2)) +
         win_a16(2 * (cap + 1) * KM);
}

// level(i) = 1 + max level(j) over rows j swept before i and coupled to i in either direction
// (a_ij or a_ji stored, j != i); forward sweeps rows 0..n-1, backward n-1..0. Returns the number
// of levels; *max_off = the most off-diagonal entries of a row.
inline int32_t gs_level_schedule(const int32_t* ip, const int32_t* ij, int64_t n, bool backward,
                                 std::vector<int32_t>& level, int32_t* max_off) {
  std::vector<int32_t> req(n, 0);
  level.assign(n, 0);
  int32_t nlev = 0;
  *max_off = 0;
  auto before = [backward](int64_t j, int64_t i) { return backward ? j > i : j < i; };
  for (int64_t t = 0; t < n; ++t) {
    const int64_t i = backward ? n - 1 - t : t;
    int32_t L = req[i], off = 0;
    for (int32_t k = ip[i]; k < ip[i + 1]; ++k) {
      const int32_t j = ij[k];
      if (j != i && before(j, i)) L = std::max(L, level[j] + 1);
      off += j != i;
    }
    level[i] = L;
    *max_off = std::max(*max_off, off);
    for (int32_t k = ip[i]; k < ip[i + 1]; ++k) {
      const int32_t j = ij[k];
      if (j != i && before(i, j)) req[j] = std::max(req[j], L + 1);
    }
    nlev = std::max(nlev, L + 1);
  }
  return nlev;
}

// the kernel (family) one sweep direction runs: mlamg_gs_path reports these values
enum GsPath : int32_t {
  kGsPathLevels = 0,     // k_gs_level, one launch per level
  kGsPathWorkgroup = 1,  // k_gs_block: one workgroup on the CSR arrays
  kGsPathWave = 2,       // k_gs_wave
  kGsPathWring = 3,      // k_gs_wring
  kGsPathPipe = 4,       // k_gs_pipe<R, K>
  kGsPathPipeLds = 5,    // k_gs_lds<K>
  kGsPathRing = 6,       // k_gs_ring
  kGsPathWindow = 7,     // k_gs_win
};

// debugging knobs, read from the environment once per mlamg_gs_create*: MLAMG_GS_NO_WIN,
// _NO_RING, _NO_LDS, _NO_WRING, _NO_WAVE = 1 take that candidate out before planning (the next in
// gs_select_path's order is planned); MLAMG_GS_PREFER_RING=1 is MLAMG_GS_NO_WIN=1;
// MLAMG_GS_WAVE_LPR = 8 or 16 fixes k_gs_wave's lanes per row
struct GsKnobs {
  bool no_win = false, no_ring = false, no_lds = false, no_wring = false, no_wave = false;
  int wave_lpr = 0;  // 0: by the schedule
  static GsKnobs from_env();
};

struct GsStep {  // k_gs_wring's step: first position, rows (the kernel reads it as an int2)
  int32_t first, rows;
};

// the plan's scalars: what the handle (gs.hpp) keeps of a plan once its arrays are uploaded
struct GsScalars {
  int64_t n = 0;
  bool backward = false;  // rows swept n-1..0
  int32_t n_levels = 0, max_level_rows = 0, max_off = 0, max_len = 0;
  int32_t K = 0;  // slots per row of a packed copy (4 or 8), 0: rows too long
  // the candidates that are planned; gs_select_path chooses among them
  bool packed = false, window = false, ring = false, pipe_lds = false, wring = false, wave = false;
  int32_t wave_lpr = 0, wave_epl = 0;  // k_gs_wave<LPR, EPL>
  // k_gs_ring: levels [l - ring_w, l] in a ring of 2^ring_log2_r slots
  int32_t ring_w = 0, ring_log2_r = 0;
  size_t ring_lds = 0;
  // k_gs_wring: SPAN = wr_lpr * wr_epl slots per position, ring horizon wr_w levels
  int32_t wr_lpr = 0, wr_epl = 0, wr_w = 0, wr_log2 = 0, wr_steps = 0;
  size_t wr_lds = 0;
  // k_gs_win: win_rw 64-row slots per level, couplings at most win_w levels apart, chunks of
  // <= win_cap positions, ring of 2^ring_log2 slots
  int32_t win_rw = 0, win_w = 0, win_cap = 0, ring_log2 = 0, n_chunks = 0;
  size_t win_lds = 0;
  GsPath path = kGsPathLevels;
};

struct GsPlan : GsScalars {
  // rows grouped by level, ascending within a level in either direction; position p = the p-th
  // row of `rows`
  std::vector<int32_t> level, level_ptr, rows;
  // packed copy: off-diagonal columns (-1 pads) and values in stored order, the last stored
  // diagonal (Dinv for block_gauss_seidel)
  std::vector<int32_t> pcol;
  std::vector<double> pval, pdiag;
  std::vector<int32_t> wpos;  // k_gs_wave: (row, first entry, length, 0) per position
  // k_gs_ring: rcol = ring position of an earlier-swept column, -(c + 2) of a later-swept one,
  // -1 pad; rcode its 16-bit code
  std::vector<int32_t> rcol;
  std::vector<uint16_t> rcode;
  std::vector<int32_t> wr_code, wr_len;  // k_gs_wring: SPAN codes and the length per position
  std::vector<GsStep> wr_st;
  // k_gs_win: wcol = the packed columns as positions; clev = 8 ints per chunk {levels, first
  // position, positions, old-x start, old-x count, level-start offset, -, -}, then every chunk's
  // level starts relative to its first position
  std::vector<int32_t> wcol, clev;
};

// Planning has two phases. The level schedule and its scalars from the matrix structure alone;
// P.packed then says whether the layouts need A's values (they are downloaded only then) ...
void gs_plan_structure(const int32_t* ip, const int32_t* ij, int64_t n, bool backward,
                       GsPlan& P);
// ... and the candidates' layouts (ax may be nullptr unless P.packed; block: pdiag holds Dinv),
// with the path chosen among them
void gs_plan_layouts(const int32_t* ip, const int32_t* ij, const double* ax, bool block,
                     const GsKnobs& knobs, GsPlan& P);
// the first candidate that is planned, in the order WINDOW, RING, PIPE_LDS, PIPE, WRING, WAVE,
// WORKGROUP, LEVELS
GsPath gs_select_path(const GsScalars& P);

}  // namespace mlamg
