// Host planner of the Gauss-Seidel sweeps (gs.hip): the level schedule of one sweep direction,
// the layouts of the kernels that can take it, and which of them runs. Plain C++: gs.hip uploads
// the plan and dispatches on its path; tests/test_gs_plan_host.py checks it without a device.
#include "gs_plan.hpp"

#include <cstdlib>

namespace mlamg {

GsKnobs GsKnobs::from_env() {
  auto on = [](const char* name) {
    const char* e = std::getenv(name);
    return e && e[0] == '1';
  };
  GsKnobs k;
  k.no_win = on("MLAMG_GS_NO_WIN") || on("MLAMG_GS_PREFER_RING");
  k.no_ring = on("MLAMG_GS_NO_RING");
  k.no_lds = on("MLAMG_GS_NO_LDS");
  k.no_wring = on("MLAMG_GS_NO_WRING");
  k.no_wave = on("MLAMG_GS_NO_WAVE");
  if (const char* e = std::getenv("MLAMG_GS_WAVE_LPR")) k.wave_lpr = e[0] == '8' ? 8 : 16;
  return k;
}

namespace {

int ceil_log2(int64_t v) {
  int lg = 0;
  while ((int64_t(1) << lg) < v) ++lg;
  return lg;
}

// pos[rows[p]] = p
std::vector<int32_t> positions(const std::vector<int32_t>& rows) {
  std::vector<int32_t> pos(rows.size());
  for (size_t p = 0; p < rows.size(); ++p) pos[rows[p]] = (int32_t)p;
  return pos;
}

// the most positions levels [l - w, l] hold, over l
int64_t widest_span(const std::vector<int32_t>& lp, int w) {
  const int nlev = (int)lp.size() - 1;
  int64_t span = 0;
  for (int l = 0; l < nlev; ++l) span = std::max<int64_t>(span, lp[l + 1] - lp[std::max(0, l - w)]);
  return span;
}

// W: the widest level distance from a row to a coupled column of an earlier level, or (both)
// of any level
int level_reach(const int32_t* ip, const int32_t* ij, const GsPlan& P, bool both) {
  const std::vector<int32_t>& level = P.level;
  int W = 0;
  for (int64_t i = 0; i < P.n; ++i)
    for (int32_t k = ip[i]; k < ip[i + 1]; ++k) {
      if (ij[k] == i) continue;
      const int d = level[i] - level[ij[k]];
      W = std::max(W, both ? std::abs(d) : d);
    }
  return W;
}

// The windowed one-wave sweep's plan: W = the widest level distance of a coupling, chunks of
// levels that fit a staging buffer, and the ring that holds every position a step and the
// concurrent staging of the next chunk touch. Not planned when levels are wider than 64 * 8 rows
// or the ring and buffers do not fit the LDS budget.
void plan_window(const int32_t* ip, const int32_t* ij, GsPlan& P) {
  const int nlev = P.n_levels, K = P.K;
  const int rw = (P.max_level_rows + 63) / 64;  // 64-row slots: <= 4 waves x 2 rows per lane
  if (rw < 1 || rw > 8 || nlev <= 4) return;
  const int W = level_reach(ip, ij, P, true);
  const std::vector<int32_t>& lp = P.level_ptr;
  for (int cap = 4096; cap >= P.max_level_rows; cap = cap * 7 / 8) {
    std::vector<int32_t> clev{0};
    for (int l = 0; l < nlev;) {
      const int start = l;
      while (l < nlev && (l == start || lp[l + 1] - lp[start] <= cap)) ++l;
      clev.push_back(l);
    }
    const int nch = (int)clev.size() - 1;
    int64_t span = 0;
    for (int ch = 0; ch < nch; ++ch) {
      const int lo = std::max(0, clev[ch] - W);
      const int hi = std::min(nlev, clev[std::min(ch + 2, nch)] + W);
      span = std::max<int64_t>(span, lp[hi] - lp[lo]);
    }
    const int lg = ceil_log2(span);
    const size_t ring = ((size_t(1) << lg) + 4) * 8;
    const size_t bufs = 2 * (size_t)win_buf_bytes(cap, K);
    if (ring + bufs > kGsWinLdsMax) continue;
    P.clev.assign(8 * (size_t)nch, 0);
    for (int ch = 0; ch < nch; ++ch) {
      const int l0 = clev[ch], l1 = clev[ch + 1];
      const int la = ch == 0 ? 0 : std::min(nlev, l0 + W), lb = std::min(nlev, l1 + W);
      const int32_t d[6] = {l1 - l0,  lp[l0],          lp[l1] - lp[l0],
                            lp[la],   lp[lb] - lp[la], (int32_t)P.clev.size() - 8 * nch};
      std::copy(d, d + 6, P.clev.begin() + 8 * (size_t)ch);
      for (int l = l0; l <= l1; ++l) P.clev.push_back(lp[l] - lp[l0]);
    }
    const std::vector<int32_t> pos = positions(P.rows);
    P.wcol.assign(P.pcol.size(), -1);
    for (size_t q = 0; q < P.pcol.size(); ++q)
      if (P.pcol[q] >= 0) P.wcol[q] = pos[P.pcol[q]];
    P.win_w = W;
    P.win_cap = cap;
    P.ring_log2 = lg;
    P.n_chunks = nch;
    P.win_lds = ring + bufs + 64;
    P.win_rw = rw;
    P.window = true;
    return;
  }
}

// The long-row ring sweep's plan (rows of 9..64 entries, levels swept in steps of 1024 / LPR
// rows): the slot codes in the padded level order, the row lengths, the step table and the ring
// (Wr levels of positions, <= 8,192 slots).
void plan_wring(const int32_t* ip, const int32_t* ij, GsPlan& P) {
  const int64_t n = P.n;
  const int nlev = P.n_levels, ml = P.max_len;
  if (n == 0 || nlev <= 4 || ml > 64) return;
  // 8 lanes per row when levels average more than 64 rows, else 16; two slots per lane in
  // 1024-thread workgroups, four (rows of 33..64 entries, or 17..32 on wide levels) in 512-thread
  // ones: five register sets of four slots exceed the 128 VGPRs a 1024-thread workgroup has
  // (spilled, the 3-D 128^3 level-1 sweep ran 2x slower than k_gs_wave)
  const bool wide = n > 64 * (int64_t)nlev;
  const int lpr = (wide && ml <= 32) ? 8 : 16;
  const int epl = ml <= 2 * lpr ? 2 : 4;
  if (ml > lpr * epl) return;
  const int span = lpr * epl, rows_per_step = (epl == 2 ? 1024 : 512) / lpr;
  const std::vector<int32_t>& lp = P.level_ptr;
  std::vector<GsStep> st;
  for (int l = 0; l < nlev; ++l)
    for (int32_t a = lp[l]; a < lp[l + 1]; a += rows_per_step)
      st.push_back(GsStep{a, std::min<int32_t>(rows_per_step, lp[l + 1] - a)});
  // a step costs about what one of k_gs_wave's level passes does: levels much wider than a step
  // stay there (3-D 128^3 level 1, 14 steps a level: V-cycle 63 -> 137 ms through this kernel)
  if (st.size() > 2 * (size_t)nlev) return;
  const size_t rest = sizeof(double) * 3 +
                      (sizeof(double) + sizeof(uint16_t)) * rows_per_step * span + 8 +
                      sizeof(GsStep) * st.size() + 16;
  if (rest >= kGsWringLdsMax) return;
  int64_t cap = int64_t(1) << kGsRingMaxLog2;  // ring slots: what the LDS budget leaves of them
  while (cap > 1 && rest + sizeof(double) * cap > kGsWringLdsMax) cap >>= 1;
  // the ring horizon Wr: the most levels back whose positions fit the ring; couplings further
  // back are read from xl two steps ahead, which needs Wr >= 2 (a step advances <= 1 level)
  const int W = level_reach(ip, ij, P, false);
  int Wr = W;
  while (Wr > 2 && widest_span(lp, Wr) > cap) Wr = std::max(2, Wr * 7 / 8);
  const int64_t spanp = widest_span(lp, Wr);
  if (spanp > cap || (Wr < W && Wr < 2)) return;
  const int lg = ceil_log2(spanp);
  if (lg > kGsRingMaxLog2 || (int64_t(1) << lg) > cap) return;
  const int32_t RM = (1 << lg) - 1;
  const std::vector<int32_t> pos = positions(P.rows);
  const std::vector<int32_t>& level = P.level;
  P.wr_code.assign((size_t)n * span, kGsWringPad);
  P.wr_len.resize(n);
  for (int64_t p = 0; p < n; ++p) {
    const int32_t i = P.rows[p];
    P.wr_len[p] = ip[i + 1] - ip[i];
    for (int32_t k = ip[i]; k < ip[i + 1]; ++k) {
      const int32_t j = ij[k];
      int32_t c = kGsWringLater;
      if (j == i) c = kGsWringDiag;
      else if (level[j] < level[i]) c = level[i] - level[j] <= Wr ? (pos[j] & RM) : kGsWringFar - pos[j];
      P.wr_code[(size_t)p * span + (k - ip[i])] = c;
    }
  }
  P.wr_st = std::move(st);
  P.wr_steps = (int32_t)P.wr_st.size();
  P.wr_lpr = lpr;
  P.wr_epl = epl;
  P.wr_w = Wr;
  P.wr_log2 = lg;
  P.wr_lds = rest + (sizeof(double) << lg);
  P.wring = true;
}

// k_gs_wave's positions and its lanes per row / entries per lane: 8 lanes per row when the levels
// average more than 64 rows (128 rows per pass: fewer passes, each with its loads on the
// critical path), else 16 (fewer entries per lane)
void plan_wave(const int32_t* ip, const GsKnobs& knobs, GsPlan& P) {
  P.wpos.resize((size_t)P.n * 4);
  for (int64_t p = 0; p < P.n; ++p) {
    const int32_t i = P.rows[p];
    const int32_t w[4] = {i, ip[i], ip[i + 1] - ip[i], 0};
    std::copy(w, w + 4, P.wpos.begin() + 4 * p);
  }
  const bool wide = knobs.wave_lpr ? knobs.wave_lpr == 8 : P.n > 64 * (int64_t)P.n_levels;
  P.wave_lpr = wide && P.max_len <= 64 ? 8 : 16;
  P.wave_epl = 1;
  while (P.wave_lpr * P.wave_epl < P.max_len) P.wave_epl *= 2;
  P.wave = true;
}

// The ring sweep's plan (levels of <= 1024 rows, K = 4 slots): W = the widest level distance from
// a row to an earlier-swept column; positions of levels [l - W, l] must fit the ring
// (<= 8,192 doubles) and the ring, its sink slot and the level starts the LDS budget.
void plan_ring(const int32_t* ip, const int32_t* ij, GsPlan& P) {
  if (P.K != kGsRingK || P.max_level_rows > kGsBlock || P.n_levels <= 4 || P.n == 0) return;
  const int W = level_reach(ip, ij, P, false);
  const int lg = ceil_log2(widest_span(P.level_ptr, W));
  const size_t lds = (sizeof(double) << lg) + sizeof(double) + sizeof(int32_t) * (P.n_levels + 1);
  if (lg > kGsRingMaxLog2 || lds > kGsRingLdsMax) return;
  const std::vector<int32_t> pos = positions(P.rows);
  const int32_t RM = (1 << lg) - 1;
  P.rcol.resize(P.pcol.size());
  P.rcode.resize(P.pcol.size());
  for (size_t e = 0; e < P.pcol.size(); ++e) {
    const int32_t c = P.pcol[e], i = P.rows[e / kGsRingK];
    const int32_t rc = c < 0 ? -1 : (P.level[c] < P.level[i] ? pos[c] : -(c + 2));
    P.rcol[e] = rc;
    P.rcode[e] = (uint16_t)(rc >= 0 ? (rc & RM) : (rc == -1 ? kGsRingPad : kGsRingLater));
  }
  P.ring_w = W;
  P.ring_log2_r = lg;
  P.ring_lds = lds;
  P.ring = true;
}

}  // namespace

GsPath gs_select_path(const GsScalars& P) {
  const bool deep = P.n_levels > 4;  // fewer levels: a launch per level costs less than the walk
  if (P.packed && deep) {
    if (P.window) return kGsPathWindow;
    if (P.ring) return kGsPathRing;
    return P.pipe_lds ? kGsPathPipeLds : kGsPathPipe;
  }
  if (P.wring) return kGsPathWring;
  if (P.wave && deep && P.max_level_rows <= kGsBlockMaxLevelRows) return kGsPathWave;
  if (deep && P.max_level_rows <= kGsBlock) return kGsPathWorkgroup;
  return kGsPathLevels;
}

void gs_plan_structure(const int32_t* ip, const int32_t* ij, int64_t n, bool backward,
                       GsPlan& P) {
  P = GsPlan();
  P.n = n;
  P.backward = backward;
  P.n_levels = gs_level_schedule(ip, ij, n, backward, P.level, &P.max_off);
  P.level_ptr.assign(P.n_levels + 1, 0);
  for (int64_t i = 0; i < n; ++i) P.level_ptr[P.level[i] + 1]++;
  for (int32_t l = 0; l < P.n_levels; ++l) {
    P.max_level_rows = std::max(P.max_level_rows, P.level_ptr[l + 1]);
    P.level_ptr[l + 1] += P.level_ptr[l];
  }
  P.rows.resize(n);
  std::vector<int32_t> fill(P.level_ptr.begin(), P.level_ptr.end() - 1);
  for (int64_t i = 0; i < n; ++i) P.rows[fill[P.level[i]]++] = (int32_t)i;
  for (int64_t i = 0; i < n; ++i) P.max_len = std::max(P.max_len, ip[i + 1] - ip[i]);
  P.K = P.max_off <= 4 ? 4 : (P.max_off <= 8 ? 8 : 0);
  // the packed copy serves one-workgroup sweeps only: levels wider than they take are swept one
  // launch per level straight from the CSR arrays, so such schedules skip it, and with it the
  // download of A's values (C4-size operators: ~1 GB of host packing and upload per sweep
  // direction)
  P.packed = P.K && P.max_level_rows <= 2 * kGsBlock;
}

void gs_plan_layouts(const int32_t* ip, const int32_t* ij, const double* ax, bool block,
                     const GsKnobs& knobs, GsPlan& P) {
  const int64_t n = P.n;
  if (!P.K && P.max_len <= 8 * kGsWaveMaxLPR && P.max_level_rows <= kGsBlockMaxLevelRows) {
    if (!knobs.no_wave) plan_wave(ip, knobs, P);
    if (!knobs.no_wring) plan_wring(ip, ij, P);
  }
  if (P.packed) {
    // level-ordered packed copy (rows with <= 8 off-diagonals)
    const int K = P.K;
    P.pcol.assign((size_t)n * K, -1);
    P.pval.assign((size_t)n * K, 0.0);
    P.pdiag.assign(n, 0.0);
    for (int64_t p = 0; p < n; ++p) {
      const int32_t i = P.rows[p];
      int c = 0;
      for (int32_t k = ip[i]; k < ip[i + 1]; ++k) {
        if (ij[k] == i) {
          P.pdiag[p] = ax[k];  // the last stored diagonal entry counts, as in the sweep
        } else {
          P.pcol[(size_t)p * K + c] = ij[k];
          P.pval[(size_t)p * K + c] = ax[k];
          ++c;
        }
      }
      if (block) P.pdiag[p] = P.pdiag[p] != 0.0 ? 1.0 / P.pdiag[p] : 0.0;  // Dinv = pinv(A_ii)
    }
    P.pipe_lds = !knobs.no_lds && P.max_level_rows <= kGsBlock && n <= kGsLdsMax;
    if (!knobs.no_win) plan_window(ip, ij, P);
    if (!P.window && !knobs.no_ring) plan_ring(ip, ij, P);
  }
  P.path = gs_select_path(P);
}

}  // namespace mlamg
