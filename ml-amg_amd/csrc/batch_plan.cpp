// The host side of the batched two-level solver (batch.hip): everything derived from the callers'
// CSR index arrays before a launch. Validation, the per-pattern structure analysis (level
// schedule, transposed sparsity of P, packed layouts, symmetry pairing, band) with its caches, the
// choice of kernel variant per problem (gs_rw, gs_db, gs_rp, panel, chol_nb, band_ld, phased,
// setup_mode) and the place of every byte of the arena. Integer work on host threads only: no HIP,
// no device, no library error state, so it builds and runs on a CPU (tests/host).
#include "batch_plan.hpp"
#include "gs_plan.hpp"

#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>

namespace mlamg {
namespace {

// A/B and diagnostic knobs of the environment, in one place
struct Knobs {
  // read once per process
  bool timing = false, no_db = false, no_rp = false;
  int ext_min = kExtCoarseMin, host_threads = 1;
  // read on every call
  bool no_cache = false, no_band = false, no_ext = false, no_phased_batch = false,
       no_phased = false, no_batch_ext = false;
};

Knobs read_knobs() {
  auto set = [](const char* name) { return std::getenv(name) != nullptr; };
  static const Knobs once = [&] {
    Knobs k;
    k.timing = set("MLAMG_BATCH_TIMING");
    k.no_db = set("MLAMG_BATCH_NO_DB");
    k.no_rp = set("MLAMG_BATCH_NO_RP");
    if (const char* e = std::getenv("MLAMG_BATCH_EXT_MIN")) k.ext_min = std::atoi(e);
    // default: the CPUs this process may run on, at most 16
    int t = 16;
    cpu_set_t cpus;
    if (sched_getaffinity(0, sizeof(cpus), &cpus) == 0) t = std::min(t, CPU_COUNT(&cpus));
    if (const char* e = std::getenv("MLAMG_HOST_THREADS")) t = std::max(1, std::atoi(e));
    k.host_threads = std::max(1, t);
    return k;
  }();
  Knobs k = once;
  k.no_cache = set("MLAMG_BATCH_NO_SHAPE_CACHE");
  k.no_band = set("MLAMG_BATCH_NO_BAND");
  k.no_ext = set("MLAMG_BATCH_NO_EXT");
  k.no_phased_batch = set("MLAMG_BATCH_NO_PHASED_BATCH");
  k.no_phased = set("MLAMG_BATCH_NO_PHASED");
  k.no_batch_ext = set("MLAMG_BATCH_NO_BATCH_EXT");
  return k;
}

struct Layout {
  size_t off = 0;
  int64_t take(size_t bytes) {
    const int64_t o = (int64_t)off;
    off += (std::max<size_t>(bytes, 1) + 255) & ~size_t(255);
    return o;
  }
};

bool valid_csr(int64_t rows, int64_t cols, int64_t nnz, const int32_t* ip, const int32_t* ij) {
  if (!ip || (nnz > 0 && !ij) || ip[0] != 0 || ip[rows] != nnz) return false;
  for (int64_t i = 0; i < rows; ++i)
    if (ip[i + 1] < ip[i]) return false;
  for (int64_t k = 0; k < nnz; ++k)
    if (ij[k] < 0 || ij[k] >= cols) return false;
  return true;
}

// the transpose of a CSR pattern by entry: column j's entries are tp[j] .. tp[j + 1], in
// ascending row; tr their rows, tk their positions in the CSR arrays
void transpose_entries(int64_t rows, int64_t cols, const int32_t* ip, const int32_t* ij,
                       std::vector<int32_t>& tp, std::vector<int32_t>& tr,
                       std::vector<int32_t>& tk) {
  const int64_t nnz = ip[rows];
  tp.assign(cols + 1, 0);
  tr.resize(nnz);
  tk.resize(nnz);
  for (int64_t k = 0; k < nnz; ++k) tp[ij[k] + 1]++;
  for (int64_t j = 0; j < cols; ++j) tp[j + 1] += tp[j];
  std::vector<int32_t> fill(tp.begin(), tp.end() - 1);
  for (int64_t i = 0; i < rows; ++i)
    for (int32_t k = ip[i]; k < ip[i + 1]; ++k) {
      tr[fill[ij[k]]] = (int32_t)i;
      tk[fill[ij[k]]++] = k;
    }
}

// A == A^T exactly (values included): then A_H = P^T A P is symmetric and, A being SPD, the
// coarse solve can take the inverse Cholesky factor
bool csr_symmetric(int64_t n, const int32_t* ip, const int32_t* ij, const double* v) {
  std::vector<int32_t> tp, tr, tk;
  transpose_entries(n, n, ip, ij, tp, tr, tk);
  // row i of A^T lists its columns ascending; compare with row i of A sorted by column
  std::vector<std::pair<int32_t, double>> row;
  for (int64_t i = 0; i < n; ++i) {
    if (ip[i + 1] - ip[i] != tp[i + 1] - tp[i]) return false;
    row.clear();
    for (int32_t k = ip[i]; k < ip[i + 1]; ++k) row.emplace_back(ij[k], v[k]);
    std::sort(row.begin(), row.end(),
              [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) {
                return a.first < b.first;
              });
    for (size_t q = 0; q < row.size(); ++q)
      if (row[q].first != tr[tp[i] + q] || !(row[q].second == v[tk[tp[i] + q]])) return false;
  }
  return true;
}

// Persistent host workers for parallel_for (creating and joining 15 threads per call cost
// ~0.5 ms of a 48-grid batch). One job at a time; a caller that finds the pool busy (another
// host thread's batch) runs its loop inline.
class HostPool {
 public:
  explicit HostPool(int workers) {
    for (int t = 0; t < workers; ++t) th_.emplace_back([this] { loop(); });
  }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  int workers() const { return (int)th_.size(); }
  // f(0 .. count-1) on the workers and the calling thread; false when the pool is busy
  bool run(int count, const std::function<void(int)>& f) {
    if (getpid() != pid_) return false;  // a forked child has no workers
    std::unique_lock<std::mutex> busy(run_mu_, std::try_to_lock);
    if (!busy.owns_lock()) return false;
    {
      std::lock_guard<std::mutex> lk(mu_);
      job_ = &f;
      count_ = count;
      next_.store(0);
      active_ = (int)th_.size();
      ++gen_;
    }
    cv_.notify_all();
    for (int q = next_.fetch_add(1); q < count; q = next_.fetch_add(1)) f(q);
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [this] { return active_ == 0; });
    job_ = nullptr;
    return true;
  }

 private:
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(int)>* job;
      int count;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
        job = job_;
        count = count_;
      }
      for (int q = next_.fetch_add(1); q < count; q = next_.fetch_add(1)) (*job)(q);
      std::lock_guard<std::mutex> lk(mu_);
      if (--active_ == 0) done_cv_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_, run_mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(int)>* job_ = nullptr;
  int count_ = 0, active_ = 0;
  uint64_t gen_ = 0;
  std::atomic<int> next_{0};
  bool stop_ = false;
  pid_t pid_ = getpid();
};

int host_threads() {
  static const int max_threads = read_knobs().host_threads;
  return max_threads;
}

HostPool& host_pool() {  // one pool for every parallel_for of the process
  static HostPool pool(host_threads() - 1);
  return pool;
}

// f(0 .. count-1) on up to MLAMG_HOST_THREADS host threads; the calling thread takes a share.
// Small counts run inline.
template <class F>
void parallel_for(int count, F&& f) {
  if (host_threads() <= 1 || count < 4) {
    for (int q = 0; q < count; ++q) f(q);
    return;
  }
  const std::function<void(int)> fn = [&](int q) { f(q); };
  if (!host_pool().run(count, fn))
    for (int q = 0; q < count; ++q) f(q);
}

// ---------------------------------------------------------------- problem patterns and shapes
// Everything the host derives from a problem's index arrays alone is computed once per distinct
// sparsity pattern and kept across calls (a dataset's grids share few patterns: the reference's
// farms loop over grids of a handful of sizes); per problem only the caller's values travel
// (A.data, P.data, b, x0) and are placed into the packed layouts on the device.
//   Pattern: the arrays (for the exact match), the exact-symmetry pairing of A's entries and the
//            half-bandwidth of A_H = P^T A P — independent of the batch's flags;
//   Shape:   a pattern's level schedule, packed column layouts and value maps for one set of
//            batch flags (smoother, phased, residual in LDS, single call).
struct Pattern {
  int64_t n = 0, nc = 0, annz = 0, pnnz = 0;
  uint64_t key = 0;
  std::vector<int32_t> aip, aij, pip, pij;
  // sym[k] = index of entry (j, i) for entry k = (i, j); sym_ok false when an entry has no
  // mirror; dups when a row repeats a column (the value test then sorts, csr_symmetric)
  std::vector<int32_t> sym;
  bool sym_ok = false, dups = false;
  int band = 0;  // half-bandwidth of A_H's structure (lower part)
  size_t bytes() const { return 4 * (aip.size() + aij.size() + pip.size() + pij.size() + sym.size()); }
};

}  // namespace

struct Shape {
  std::shared_ptr<const Pattern> pat;
  int smoother = 0, phased = 0, r_lds = 0, single = 0;
  // slot-major packed columns (-1 pads) and, per slot, the index of its value in A.data /
  // P.data (-1: pad, value 0.0)
  std::vector<int32_t> akc, amap, ppc, pmap, ptc, tmap;
  // Gauss-Seidel sweep in level order: lev/clev (level and chunk starts), pkc/gmap the
  // off-diagonal slots (position-major for the one-wave sweep), dmap the last stored diagonal
  // entry of each position (-1: none), pkr0 the position's row
  std::vector<int32_t> lev, clev, pkc, gmap, dmap, pkr0;
  bool chol_fits = false;
  int K = 1, KA = 1, KP = 1, KT = 1, nlev = 0, panel = 8, cap = 0, chol_nb = 4;
  int gs_rw = 0, gs_db = 0, gs_rp = 0;
  size_t lds_base = 0, lds_chol = 0, lds_cycles = 0;
  int code = MLAMG_OK;
  std::string err;
  size_t bytes() const;
};

namespace {

// a shape's index arrays in arena order, each with the descriptor field that holds its offset:
// the one list behind Shape::bytes, the layout, the descriptors and fill_inputs
struct ShapeArray {
  std::vector<int32_t> Shape::*host;
  int64_t BDesc::*off;
};
constexpr ShapeArray kShapeArrays[] = {
    {&Shape::akc, &BDesc::ak_col},   {&Shape::amap, &BDesc::a_map},
    {&Shape::ppc, &BDesc::pp_col},   {&Shape::pmap, &BDesc::p_map},
    {&Shape::ptc, &BDesc::pt_row},   {&Shape::tmap, &BDesc::t_map},
    {&Shape::lev, &BDesc::lev_ptr},  {&Shape::clev, &BDesc::chunk_lev},
    {&Shape::pkc, &BDesc::pk_col},   {&Shape::gmap, &BDesc::g_map},
    {&Shape::dmap, &BDesc::d_map},   {&Shape::pkr0, &BDesc::pk_row0},
};

}  // namespace

size_t Shape::bytes() const {
  size_t b = 0;
  for (const ShapeArray& a : kShapeArrays) b += 4 * (this->*a.host).size();
  return b;
}

namespace {

uint64_t mix_bytes(const void* data, size_t bytes, uint64_t h) {
  const unsigned char* p = static_cast<const unsigned char*>(data);
  constexpr uint64_t M1 = 0x9E3779B97F4A7C15ull, M2 = 0xC2B2AE3D27D4EB4Full;
  uint64_t a = h ^ M1, b = h + M2, c = h * M1 + 1, d = h ^ M2;
  size_t i = 0;
  for (; i + 32 <= bytes; i += 32) {  // four independent lanes
    uint64_t w[4];
    std::memcpy(w, p + i, 32);
    a = (a ^ w[0]) * M1;
    b = (b ^ w[1]) * M2;
    c = (c ^ w[2]) * M1;
    d = (d ^ w[3]) * M2;
    a ^= a >> 29;
    b ^= b >> 31;
    c ^= c >> 27;
    d ^= d >> 33;
  }
  for (; i < bytes; ++i) a = (a ^ p[i]) * M1;
  uint64_t r = a ^ (b * M1) ^ (c * M2) ^ (d + M1) ^ bytes;
  r ^= r >> 32;
  return r * M2;
}

uint64_t pattern_key(const mlamg_amg2v_problem& P) {
  int64_t hdr[4] = {P.n, P.n_c, P.A_nnz, P.P_nnz};
  uint64_t h = mix_bytes(hdr, sizeof(hdr), 0x5A17u);
  h = mix_bytes(P.A_indptr, 4 * (size_t)(P.n + 1), h);
  h = mix_bytes(P.A_indices, 4 * (size_t)P.A_nnz, h);
  h = mix_bytes(P.P_indptr, 4 * (size_t)(P.n + 1), h);
  return mix_bytes(P.P_indices, 4 * (size_t)P.P_nnz, h);
}

bool same_pattern(const mlamg_amg2v_problem& a, const mlamg_amg2v_problem& b) {
  if (a.n != b.n || a.n_c != b.n_c || a.A_nnz != b.A_nnz || a.P_nnz != b.P_nnz) return false;
  auto eq = [](const int32_t* x, const int32_t* y, int64_t cnt) {
    return x == y || cnt == 0 || std::memcmp(x, y, 4 * (size_t)cnt) == 0;
  };
  return eq(a.A_indptr, b.A_indptr, a.n + 1) && eq(a.A_indices, b.A_indices, a.A_nnz) &&
         eq(a.P_indptr, b.P_indptr, a.n + 1) && eq(a.P_indices, b.P_indices, a.P_nnz);
}

bool pattern_matches(const Pattern& S, const mlamg_amg2v_problem& P) {
  mlamg_amg2v_problem q{};
  q.n = S.n;
  q.n_c = S.nc;
  q.A_nnz = S.annz;
  q.P_nnz = S.pnnz;
  q.A_indptr = S.aip.data();
  q.A_indices = S.aij.data();
  q.P_indptr = S.pip.data();
  q.P_indices = S.pij.data();
  return same_pattern(q, P);
}

// bounded most-recently-used lists (count and bytes); one lock for both
std::mutex g_shape_mu;
std::vector<std::shared_ptr<const Pattern>> g_patterns;
std::vector<std::shared_ptr<const Shape>> g_shapes;
constexpr size_t kCacheCount = 64;
constexpr size_t kCacheBytes = size_t(256) << 20;

template <class T>
void cache_trim(std::vector<std::shared_ptr<const T>>& v) {
  size_t total = 0;
  for (const auto& t : v) total += t->bytes();
  while (v.size() > 1 && (v.size() > kCacheCount || total > kCacheBytes)) {
    total -= v.front()->bytes();
    v.erase(v.begin());
  }
}

std::shared_ptr<const Pattern> pattern_lookup(uint64_t key, const mlamg_amg2v_problem& P) {
  std::lock_guard<std::mutex> lk(g_shape_mu);
  for (size_t i = g_patterns.size(); i-- > 0;)
    if (g_patterns[i]->key == key && pattern_matches(*g_patterns[i], P)) {
      auto s = g_patterns[i];
      g_patterns.erase(g_patterns.begin() + (long)i);
      g_patterns.push_back(s);
      return s;
    }
  return nullptr;
}

std::shared_ptr<const Shape> shape_lookup(const Pattern* pat, int smoother, int phased,
                                          int r_lds, int single) {
  std::lock_guard<std::mutex> lk(g_shape_mu);
  for (size_t i = g_shapes.size(); i-- > 0;) {
    const Shape& S = *g_shapes[i];
    if (S.pat.get() == pat && S.smoother == smoother && S.phased == phased &&
        S.r_lds == r_lds && S.single == single) {
      auto s = g_shapes[i];
      g_shapes.erase(g_shapes.begin() + (long)i);
      g_shapes.push_back(s);
      return s;
    }
  }
  return nullptr;
}

void pattern_insert(const std::shared_ptr<const Pattern>& s) {
  std::lock_guard<std::mutex> lk(g_shape_mu);
  g_patterns.push_back(s);
  cache_trim(g_patterns);
}

void shape_insert(const std::shared_ptr<const Shape>& s) {
  std::lock_guard<std::mutex> lk(g_shape_mu);
  g_shapes.push_back(s);
  cache_trim(g_shapes);
}

// rows of a CSR pattern into a slot-major fixed-width layout: col (-1 pads) and the index of
// each slot's value (-1 pads); width = the longest row (>= 1)
int pack_map(int64_t rows, const int32_t* ip, const int32_t* ij, std::vector<int32_t>& col,
             std::vector<int32_t>& map) {
  int w = 1;
  for (int64_t i = 0; i < rows; ++i) w = std::max(w, ip[i + 1] - ip[i]);
  col.assign((size_t)w * rows, -1);
  map.assign((size_t)w * rows, -1);
  for (int64_t i = 0; i < rows; ++i)
    for (int32_t k = ip[i]; k < ip[i + 1]; ++k) {
      col[(size_t)(k - ip[i]) * rows + i] = ij[k];
      map[(size_t)(k - ip[i]) * rows + i] = k;
    }
  return w;
}

std::shared_ptr<Pattern> analyse_pattern(const mlamg_amg2v_problem& P, uint64_t key) {
  auto Sp = std::make_shared<Pattern>();
  Pattern& S = *Sp;
  const int64_t n = P.n, nnz = P.A_nnz;
  const int32_t *ip = P.A_indptr, *ij = P.A_indices;
  S.n = n;
  S.nc = P.n_c;
  S.annz = nnz;
  S.pnnz = P.P_nnz;
  S.key = key;
  S.aip.assign(ip, ip + n + 1);
  S.aij.assign(ij, ij + nnz);
  S.pip.assign(P.P_indptr, P.P_indptr + n + 1);
  S.pij.assign(P.P_indices, P.P_indices + P.P_nnz);
  // A's structural transpose pairing
  std::vector<int32_t> tp, tr, tk;
  transpose_entries(n, n, ip, ij, tp, tr, tk);
  S.sym.assign(nnz, -1);
  S.sym_ok = true;
  std::vector<std::pair<int32_t, int32_t>> row;
  for (int64_t i = 0; i < n; ++i) {
    row.clear();
    for (int32_t k = ip[i]; k < ip[i + 1]; ++k) row.emplace_back(ij[k], k);
    std::sort(row.begin(), row.end());
    for (size_t q = 1; q < row.size(); ++q)
      if (row[q].first == row[q - 1].first) S.dups = true;
    if (ip[i + 1] - ip[i] != tp[i + 1] - tp[i]) {
      S.sym_ok = false;
      continue;
    }
    // column i of A (entries (r, i), r ascending) against row i's columns ascending
    for (size_t q = 0; q < row.size(); ++q) {
      if (tr[tp[i] + q] != row[q].first) S.sym_ok = false;
      S.sym[row[q].second] = tk[tp[i] + q];
    }
  }
  if (S.dups) S.sym_ok = false;
  // half-bandwidth of A_H: (P^T A P)_IJ != 0 needs P_iI, A_ik, P_kJ != 0, so the lowest J of
  // any coarse row I of fine row i is the lowest P column over i's A neighbours
  std::vector<int32_t> pmin(n, INT32_MAX);
  for (int64_t i = 0; i < n; ++i)
    for (int32_t k = P.P_indptr[i]; k < P.P_indptr[i + 1]; ++k)
      pmin[i] = std::min(pmin[i], P.P_indices[k]);
  int band = 0;
  for (int64_t i = 0; i < n; ++i) {
    int32_t am = INT32_MAX;
    for (int32_t k = ip[i]; k < ip[i + 1]; ++k) am = std::min(am, pmin[ij[k]]);
    if (am == INT32_MAX) continue;
    for (int32_t k = P.P_indptr[i]; k < P.P_indptr[i + 1]; ++k)
      band = std::max(band, P.P_indices[k] - am);
  }
  S.band = band;
  return Sp;
}

// the Gauss-Seidel part of a shape: levels (rows ascending within a level), the sweep variant
// and its packed rows; `room` is the LDS left for the staging area. False: refused (L.code set)
bool analyse_sweep(const mlamg_amg2v_problem& P, size_t room, bool no_db, Shape& L) {
  const int64_t n = P.n;
  std::vector<int32_t> level;
  int32_t maxoff = 0;  // the forward sweep's level recurrence (gs_plan.hpp)
  L.nlev = gs_level_schedule(P.A_indptr, P.A_indices, n, false, level, &maxoff);
  if (maxoff > kBMaxK) {
    L.code = MLAMG_EUNSUPPORTED;
    L.err = "amg2v_batch: a row of A has more than 32 off-diagonal entries";
    return false;
  }
  L.lev.assign(L.nlev + 1, 0);
  for (int64_t i = 0; i < n; ++i) L.lev[level[i] + 1]++;
  for (int l = 0; l < L.nlev; ++l) L.lev[l + 1] += L.lev[l];
  int wmax = 0;
  for (int l = 0; l < L.nlev; ++l) wmax = std::max(wmax, L.lev[l + 1] - L.lev[l]);
  // one-wave sweep: rows of 4 slots and levels of <= 128 rows, or 8 slots and <= 64 rows,
  // and a staging area that holds the widest level (+ the dummy position)
  const int km = maxoff <= 4 ? 4 : maxoff <= 8 ? 8 : 0;
  int gs_rw = 0;
  if (km == 4 && wmax <= 128) gs_rw = wmax <= 64 ? 1 : 2;
  if (km == 8 && wmax <= 64) gs_rw = 1;
  if (gs_rw && (int)std::min<size_t>(4096, room / stage_pos_lds(km, false)) - 1 < wmax) gs_rw = 0;
  // two staging buffers when each still holds >= 3 of the widest levels
  if (gs_rw && !no_db &&
      (int)std::min<size_t>(4096, room / (stage_pos_lds(km, true) + 16)) - 1 >= 3 * wmax)
    L.gs_db = 1;
  L.gs_rw = gs_rw;
  L.K = gs_rw ? km : std::max(maxoff, 1);
  const int64_t K = L.K;
  L.pkr0.resize(n);
  L.pkc.assign((size_t)n * K, gs_rw ? (int32_t)n : -1);
  L.gmap.assign((size_t)n * K, -1);
  L.dmap.assign(n, -1);
  std::vector<int32_t> fill(L.lev.begin(), L.lev.end() - 1);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t p = fill[level[i]]++;
    L.pkr0[p] = (int32_t)i;
    int s2 = 0;
    for (int32_t k = P.A_indptr[i]; k < P.A_indptr[i + 1]; ++k) {
      if (P.A_indices[k] == i) {
        L.dmap[p] = k;  // the last stored diagonal entry, as the sweep takes it
      } else {
        // slot-major for the workgroup sweep, position-major for the one-wave sweep
        const size_t at = gs_rw ? (size_t)p * K + s2 : (size_t)s2 * n + p;
        L.pkc[at] = P.A_indices[k];
        L.gmap[at] = k;
        ++s2;
      }
    }
  }
  return true;
}

// GS staging chunks: runs of consecutive levels with <= cap rows, cap from the LDS left after
// the cycle vectors, one position kept for the one-wave sweep's dummy (a level wider than cap is
// swept by the workgroup straight from the arena)
void chunk_levels(size_t room, Shape& L) {
  const size_t slack = L.gs_db ? 32 : 0;
  L.cap = (int)std::min<size_t>(4096, (room > slack ? room - slack : 0) /
                                          stage_pos_lds(L.K, L.gs_db != 0)) - 1;
  L.clev.push_back(0);
  int l = 0;
  while (l < L.nlev) {
    const int start = l;
    int cnt = 0;
    while (l < L.nlev && (l == start || cnt + (L.lev[l + 1] - L.lev[l]) <= L.cap)) {
      cnt += L.lev[l + 1] - L.lev[l];
      ++l;
    }
    L.clev.push_back(l);
  }
}

// the structure analysis of one pattern (P already validated)
std::shared_ptr<Shape> analyse_shape(const mlamg_amg2v_problem& P,
                                     const std::shared_ptr<const Pattern>& pat, int smoother,
                                     int phased, int r_lds, int single, const Knobs& knobs) {
  auto Sp = std::make_shared<Shape>();
  Shape& L = *Sp;
  const int64_t n = P.n, nc = P.n_c;
  L.pat = pat;
  L.smoother = smoother;
  L.phased = phased;
  L.r_lds = r_lds;
  L.single = single;
  L.KA = pack_map(n, P.A_indptr, P.A_indices, L.akc, L.amap);
  L.KP = pack_map(n, P.P_indptr, P.P_indices, L.ppc, L.pmap);
  {  // P^T: entries of coarse column j in ascending fine row
    std::vector<int32_t> tp, ti, tk;
    transpose_entries(n, nc, P.P_indptr, P.P_indices, tp, ti, tk);
    L.KT = pack_map(nc, tp.data(), ti.data(), L.ptc, L.tmap);
    // pack_map stored positions into ti/tk; map them back to P.data indices
    for (auto& m : L.tmap)
      if (m >= 0) m = tk[m];
  }
  if (L.KA > kBMaxK + 1 || L.KP > kBMaxKP || L.KT > kBMaxKT) {
    L.code = MLAMG_EUNSUPPORTED;
    L.err = "amg2v_batch: rows of A, P or P^T longer than the batched solver's slots";
    return Sp;
  }
  int chol_nb = 16;  // the widest panel that fits (wider panels lengthen the per-thread
                     // triangular solves more than they save in trailing passes)
  while (chol_nb > 4 && chol_lds(chol_nb, nc) > kBLdsBytes) chol_nb >>= 1;
  L.chol_nb = chol_nb;
  L.chol_fits = chol_lds(chol_nb, nc) <= kBLdsBytes;
  L.lds_chol = chol_lds(chol_nb, nc);
  // the sweep's staging area gets the LDS the cycle vectors leave
  const size_t vec_lds = cycle_vec_lds(n, nc, r_lds != 0, phased != 0);
  const size_t room = kBLdsBytes > vec_lds + 64 ? kBLdsBytes - vec_lds - 64 : 0;
  if (smoother == 0 && !analyse_sweep(P, room, knobs.no_db, L)) return Sp;
  // panel width: the widest power of two <= 16 whose n_c x (b+1) panel (+ pivots and the
  // final column permutation) fits
  int pb = kBMaxPanel;
  while (pb > 4 && gj_lds(pb, nc) > kBLdsBytes) pb >>= 1;
  if (gj_lds(pb, nc) > kBLdsBytes) {
    L.code = MLAMG_EINVAL;
    L.err = "coarse too large";
    return Sp;
  }
  L.panel = pb;
  if (smoother == 0) chunk_levels(room, L);
  if (phased && single && L.gs_rw && !L.gs_db && !knobs.no_rp && L.cap + 1 <= kBT - 64 &&
      L.cap * L.K <= 2 * (kBT - 64))
    L.gs_rp = 1;
  L.lds_base = gj_lds(pb, nc);
  L.lds_cycles = cycles_lds(vec_lds, L.cap, L.K, L.gs_db != 0);
  return Sp;
}

// ---------------------------------------------------------------- the steps of plan_batch
struct Work {  // per problem, between the steps
  std::vector<uint64_t> key;
  std::vector<int> rep;  // the first problem with the same pattern (itself: a representative)
  std::vector<std::shared_ptr<const Pattern>> pat;
  std::vector<std::shared_ptr<const Shape>> shape;
  std::vector<char> sym, band, spd;
};

int refuse(BatchPlan* out, int code, const std::string& msg) {
  out->code = code;
  out->err = msg;
  return code;
}

// 1. validation and the pattern key of every problem (host threads)
int validate(const mlamg_amg2v_problem* probs, int count, int max_iter, Work& W, BatchPlan* out) {
  std::vector<const char*> verr(count, nullptr);
  W.key.assign(count, 0);
  parallel_for(count, [&](int q) {
    const mlamg_amg2v_problem& P = probs[q];
    auto fail = [&](const char* m) { verr[q] = m; };
    const int64_t n = P.n, nc = P.n_c;
    if (!(n >= 1 && n <= kBMaxN)) return fail("problem rows out of range for the batched solver");
    if (!(nc >= 1 && nc <= kBMaxNc && nc <= n)) return fail("coarse size out of range");
    if (!(valid_csr(n, n, P.A_nnz, P.A_indptr, P.A_indices) && P.A_data))
      return fail("A is not a valid n x n CSR");
    if (!(valid_csr(n, nc, P.P_nnz, P.P_indptr, P.P_indices) && P.P_data))
      return fail("P is not a valid n x n_c CSR");
    if (!(P.b && P.x0 && P.x_out && (max_iter == 0 || P.err_out))) return fail("NULL vector");
    W.key[q] = pattern_key(P);
  });
  for (int q = 0; q < count; ++q)
    if (verr[q])
      return refuse(out, MLAMG_EINVAL,
                    std::string(verr[q]) + " (problem " + std::to_string(q) + ")");
  return MLAMG_OK;
}

// 2. group by key (a representative per distinct key), members compared in full (a key
// collision leaves the member its own pattern); patterns from the cache or analysed
void find_patterns(const mlamg_amg2v_problem* probs, int count, bool no_cache, Work& W) {
  W.rep.resize(count);
  std::vector<std::pair<uint64_t, int>> order(count);
  for (int q = 0; q < count; ++q) order[q] = {W.key[q], q};
  std::sort(order.begin(), order.end());
  for (int t = 0; t < count; ++t)
    W.rep[order[t].second] = t > 0 && order[t].first == order[t - 1].first
                                 ? W.rep[order[t - 1].second]
                                 : order[t].second;
  parallel_for(count, [&](int q) {
    if (W.rep[q] != q && !same_pattern(probs[q], probs[W.rep[q]])) W.rep[q] = q;
  });
  W.pat.assign(count, nullptr);
  std::vector<int> todo;
  for (int q = 0; q < count; ++q)
    if (W.rep[q] == q) {
      if (!no_cache) W.pat[q] = pattern_lookup(W.key[q], probs[q]);
      if (!W.pat[q]) todo.push_back(q);
    }
  parallel_for((int)todo.size(), [&](int t) {
    const int q = todo[t];
    auto S = analyse_pattern(probs[q], W.key[q]);
    if (!no_cache) pattern_insert(S);
    W.pat[q] = S;
  });
  for (int q = 0; q < count; ++q) W.pat[q] = W.pat[W.rep[q]];
}

// 3. per problem: A == A^T exactly (values included) -> an SPD coarse operator, factored as a
// band when its structure is narrow, else as a dense inverse Cholesky factor
void classify(const mlamg_amg2v_problem* probs, int count, bool no_band, Work& W) {
  W.sym.assign(count, 0);
  W.band.assign(count, 0);
  parallel_for(count, [&](int q) {
    const Pattern& S = *W.pat[q];
    const mlamg_amg2v_problem& P = probs[q];
    bool s = false;
    if (S.sym_ok) {
      s = true;
      for (int64_t k = 0; k < S.annz && s; ++k) s = P.A_data[k] == P.A_data[S.sym[k]];
    } else if (S.dups) {
      s = csr_symmetric(P.n, P.A_indptr, P.A_indices, P.A_data);
    }
    W.sym[q] = s ? 1 : 0;
    W.band[q] = s && !no_band && S.band <= kBandMax && S.nc <= kBandMaxNc &&
                band_lds(S.band) <= kBLdsBytes ? 1 : 0;
  });
}

// 5. shapes for the batch's flags (cached per pattern), then the dense inverse Cholesky factor
// where no band is taken and it fits one workgroup's LDS
int find_shapes(const mlamg_amg2v_problem* probs, int count, int smoother, const Knobs& knobs,
                Work& W, BatchPlan* out) {
  const int phased = out->phased, r_lds = out->r_lds, single = count == 1 ? 1 : 0;
  W.shape.assign(count, nullptr);
  std::vector<int> todo;
  for (int q = 0; q < count; ++q)
    if (W.rep[q] == q) {
      if (!knobs.no_cache)
        W.shape[q] = shape_lookup(W.pat[q].get(), smoother, phased, r_lds, single);
      if (!W.shape[q]) todo.push_back(q);
    }
  parallel_for((int)todo.size(), [&](int t) {
    const int q = todo[t];
    auto S = analyse_shape(probs[q], W.pat[q], smoother, phased, r_lds, single, knobs);
    if (S->code == MLAMG_OK && !knobs.no_cache) shape_insert(S);
    W.shape[q] = S;
  });
  for (int q = 0; q < count; ++q) W.shape[q] = W.shape[W.rep[q]];
  for (int q = 0; q < count; ++q)
    if (W.shape[q]->code != MLAMG_OK)
      return refuse(out, W.shape[q]->code,
                    W.shape[q]->err + " (problem " + std::to_string(q) + ")");
  W.spd.assign(count, 0);
  for (int q = 0; q < count; ++q)
    W.spd[q] = W.sym[q] && !W.band[q] && W.shape[q]->chol_fits ? 1 : 0;
  return MLAMG_OK;
}

// the fields of a problem's descriptor that are not arena offsets
void describe(const Work& W, int q, const mlamg_amg2v_problem& P, const BatchPlan& plan,
              int smoother, int nu_pre, int nu_post, double jacobi_weight, int norm_mode,
              double tol, int max_iter, BDesc& D) {
  const Shape& L = *W.shape[q];
  D.n = (int32_t)P.n;
  D.nc = (int32_t)P.n_c;
  D.smoother = smoother;
  D.nu_pre = nu_pre;
  D.nu_post = nu_post;
  D.norm_mode = norm_mode;
  D.max_iter = max_iter;
  D.K = L.K;
  D.KA = L.KA;
  D.KP = L.KP;
  D.KT = L.KT;
  D.nlev = L.nlev;
  D.panel = L.panel;
  D.n_chunks = L.clev.empty() ? 0 : (int32_t)L.clev.size() - 1;
  D.cap = L.cap;
  D.timing = plan.timing ? 1 : 0;
  D.spd = W.spd[q];
  D.band_ld = W.band[q] ? W.pat[q]->band + 1 : 0;
  D.chol_nb = L.chol_nb;
  D.gs_rw = L.gs_rw;
  D.gs_db = L.gs_db;
  D.gs_rp = L.gs_rp;
  D.phased = plan.phased ? 1 : 0;
  D.tol = tol;
  D.omega = jacobi_weight;
}

// the arena's input part: descriptors, each distinct shape's structure once, every problem's
// values, the phased batch's coarse-block table
void lay_inputs(const mlamg_amg2v_problem* probs, int count, const Work& W, Layout& lay,
                BatchPlan* out) {
  std::vector<BDesc>& desc = out->desc;
  out->desc_off = lay.take(sizeof(BDesc) * count);
  for (int q = 0; q < count; ++q) {
    if (W.rep[q] != q) continue;
    for (const ShapeArray& a : kShapeArrays)
      desc[q].*a.off = lay.take(4 * ((*W.shape[q]).*a.host).size());
    out->shapes.push_back(W.shape[q]);
    out->shape_rep.push_back(q);
  }
  for (int q = 0; q < count; ++q) {
    BDesc& D = desc[q];
    for (const ShapeArray& a : kShapeArrays) D.*a.off = desc[W.rep[q]].*a.off;
    D.a_raw = lay.take(8 * (size_t)probs[q].A_nnz);
    D.p_raw = lay.take(8 * (size_t)probs[q].P_nnz);
    D.b = lay.take(8 * (size_t)D.n);
    D.x0 = lay.take(8 * (size_t)D.n);
  }
  // phased: each problem's first coarse-solve block (k_amg2v_coarse), a row per wave
  out->cblk_off = out->phased ? lay.take(4 * (size_t)(count + 1)) : 0;
  out->cblk.assign(count + 1, 0);
  for (int q = 0; q < count; ++q)
    out->cblk[q + 1] = out->cblk[q] + (int32_t)((desc[q].nc + 3) / 4);
  out->in_bytes = lay.off;
}

// the arena's device-only part (packed values, gathered on the device by gather_values; the
// coarse operator and its factor; work vectors), then the outputs
void lay_work_and_outputs(const Work& W, int count, int max_iter, Layout& lay, BatchPlan* out) {
  const bool phased = out->phased;
  for (int q = 0; q < count; ++q) {
    BDesc& D = out->desc[q];
    const Shape& L = *W.shape[q];
    D.ak_val = lay.take(8 * L.akc.size());
    D.pp_val = lay.take(8 * L.ppc.size());
    D.pt_val = lay.take(8 * L.ptc.size());
    D.pk_val = lay.take(8 * L.pkc.size());
    D.pk_diag = lay.take(8 * L.pkr0.size());
    D.pk_row = lay.take(4 * L.pkr0.size());
    D.b_lvl = lay.take(8 * L.pkr0.size());
    D.AH = lay.take((size_t)8 * D.nc * D.nc);
    D.AI = lay.take((size_t)8 * D.nc * D.nc);
    D.rg = lay.take(8 * (size_t)D.n);
    D.dinv = lay.take(8 * (size_t)D.n);
    if (D.band_ld > 0) {  // the band solve's lane layouts (band_chol), padded
      D.lc = lay.take((size_t)8 * 64 * (D.nc + 2 * kBandPad));
      D.lr = lay.take((size_t)8 * 64 * (D.nc + 2 * kBandPad));
      D.rinv = lay.take((size_t)8 * (D.nc + 2 * kBandPad));
    }
    if (phased) {
      D.rcg = lay.take(8 * (size_t)D.nc);
      D.eg = lay.take(8 * (size_t)D.nc);
      D.yg = lay.take(8 * (size_t)D.nc);
    }
  }
  out->done_off = phased ? lay.take(sizeof(int32_t)) : 0;
  for (int q = 0; q < count; ++q) out->desc[q].done_ctr = out->done_off;
  out->out_begin = lay.off;
  for (int q = 0; q < count; ++q) {
    BDesc& D = out->desc[q];
    D.x_out = lay.take(8 * (size_t)D.n);
    D.err_out = lay.take(8 * (size_t)std::max(max_iter, 1));
    D.stat_out = lay.take(16 + 8 * 8);
  }
  out->total = lay.off;
}

}  // namespace

int plan_batch(const mlamg_amg2v_problem* probs, int count, int smoother, int nu_pre, int nu_post,
               double jacobi_weight, int norm_mode, double tol, int max_iter, BatchPlan* out) {
  *out = BatchPlan();
  const Knobs knobs = read_knobs();
  out->timing = knobs.timing;
  Work W;
  if (validate(probs, count, max_iter, W, out) != MLAMG_OK) return out->code;
  find_patterns(probs, count, knobs.no_cache, W);
  classify(probs, count, knobs.no_band, W);
  // 4. strategy. A single problem with a large dense coarse operator: the coarse inverse from
  // the device-wide factorisation (dense.hip) and phased cycles, the coarse solve on every CU.
  // Batches holding such problems run phased too (each problem's cycles on its workgroup, the
  // dense coarse solves spread over the CUs; banded problems solve on their own workgroup)
  bool big_dense = false;
  for (int q = 0; q < count; ++q)
    big_dense = big_dense || (!W.band[q] && probs[q].n_c > knobs.ext_min);
  const bool ext_ok = count == 1 && big_dense && !knobs.no_ext;
  const bool phased_batch = count > 1 && big_dense && !knobs.no_ext && !knobs.no_phased_batch;
  const bool phased = out->phased = (ext_ok || phased_batch) && !knobs.no_phased;
  // residual in LDS when every problem leaves room for it (phased: r_H, e_H live in the arena)
  out->r_lds = true;
  for (int q = 0; q < count; ++q)
    if (cycle_vec_lds(probs[q].n, probs[q].n_c, true, phased) + 16 * 1024 > kBLdsBytes)
      out->r_lds = false;
  if (find_shapes(probs, count, smoother, knobs, W, out) != MLAMG_OK) return out->code;
  out->t_analysed = std::chrono::steady_clock::now();
  // ---- layout: each distinct shape's structure once, then every problem's values
  out->desc.resize(count);
  std::memset(out->desc.data(), 0, sizeof(BDesc) * count);
  for (int q = 0; q < count; ++q) {
    const Shape& L = *W.shape[q];
    out->any_band = out->any_band || W.band[q];
    out->lds_setup = std::max(out->lds_setup, std::max(L.lds_base, W.spd[q] ? L.lds_chol : 0));
    if (W.band[q]) out->lds_band = std::max(out->lds_band, band_lds(W.pat[q]->band));
    out->lds_cycles = std::max(out->lds_cycles, L.lds_cycles);
    describe(W, q, probs[q], *out, smoother, nu_pre, nu_post, jacobi_weight, norm_mode, tol,
             max_iter, out->desc[q]);
  }
  if (!(out->lds_setup <= kBLdsBytes + 1024 && out->lds_cycles <= kBLdsBytes + 1024))
    return refuse(out, MLAMG_EINVAL, "mlamg_amg2v_batch: LDS budget exceeded");
  Layout lay;
  lay_inputs(probs, count, W, lay, out);
  lay_work_and_outputs(W, count, max_iter, lay, out);
  // a single problem with a large SPD coarse operator takes the device-wide coarse factorisation
  out->ext_coarse = ext_ok && W.spd[0];
  if (out->ext_coarse) out->desc[0].setup_mode = 1;
  // a phased batch factors its large SPD operators device-wide too, all in one launch sequence.
  // The factor is chosen by the problem's own n_c, as a single call chooses it (the batched and
  // the single device-wide factors run the same code per operator): a problem's results do not
  // depend on the batch it is launched with
  out->batch_ext = phased && count > 1 && !knobs.no_batch_ext;
  if (out->batch_ext)
    for (int q = 0; q < count; ++q)
      if (W.spd[q] && out->desc[q].nc > knobs.ext_min) out->desc[q].setup_mode = 2;
  // phased: mode-1 problems (one-workgroup inverse Cholesky factor) need the second, L^-T, pass
  // of the coarse solve; a single call may take the register-prefetch sweep
  for (int q = 0; q < count && phased; ++q)
    out->two_pass = out->two_pass || (W.spd[q] && out->desc[q].setup_mode == 0);
  out->rp = phased && count == 1 && out->desc[0].gs_rp != 0;
  return MLAMG_OK;
}

void fill_inputs(const BatchPlan& plan, const mlamg_amg2v_problem* probs, char* host_buf) {
  const int count = (int)plan.desc.size(), nu = (int)plan.shapes.size();
  std::memcpy(host_buf + plan.desc_off, plan.desc.data(), sizeof(BDesc) * count);
  if (plan.phased)
    std::memcpy(host_buf + plan.cblk_off, plan.cblk.data(), 4 * (size_t)(count + 1));
  auto put = [&](int64_t off, const void* src, size_t bytes) {
    if (bytes) std::memcpy(host_buf + off, src, bytes);
  };
  parallel_for(nu + count, [&](int t) {
    if (t < nu) {  // a shape's structure
      const Shape& S = *plan.shapes[t];
      const BDesc& D = plan.desc[plan.shape_rep[t]];
      for (const ShapeArray& a : kShapeArrays)
        put(D.*a.off, (S.*a.host).data(), 4 * (S.*a.host).size());
      return;
    }
    const int q = t - nu;  // a problem's values
    const mlamg_amg2v_problem& P = probs[q];
    const BDesc& D = plan.desc[q];
    put(D.a_raw, P.A_data, 8 * (size_t)P.A_nnz);
    put(D.p_raw, P.P_data, 8 * (size_t)P.P_nnz);
    put(D.b, P.b, 8 * (size_t)P.n);
    put(D.x0, P.x0, 8 * (size_t)P.n);
  });
}

void read_outputs(const BatchPlan& plan, mlamg_amg2v_problem* probs, const char* host_out,
                  int max_iter) {
  for (size_t q = 0; q < plan.desc.size(); ++q) {
    mlamg_amg2v_problem& P = probs[q];
    const BDesc& D = plan.desc[q];
    const int32_t* st = reinterpret_cast<const int32_t*>(host_out + (D.stat_out - plan.out_begin));
    P.iters_out = st[0];
    P.status_out = st[1];
    std::memcpy(P.x_out, host_out + (D.x_out - plan.out_begin), 8 * (size_t)P.n);
    if (max_iter > 0)
      std::memcpy(P.err_out, host_out + (D.err_out - plan.out_begin), 8 * (size_t)st[0]);
  }
}

}  // namespace mlamg
