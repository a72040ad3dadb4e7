// Storage formats of the SpMV family: everything that builds, drops or describes one.
//
// Runs once per handle (mlamg_csr_set_format): the SELL, SELL-dict, sorted (with its value and
// block dictionaries), vec16, long and row-pair-pattern builders with their small build
// kernels, the one list of each format's arrays (drop_*), and the C-ABI entries that set,
// report and size a format. The kernels that read these arrays are in spmv.hip; formats.hpp is
// the seam between the two.
#include "formats.hpp"

#include <cstdlib>

#include <rocprim/rocprim.hpp>

namespace mlamg {

// Forget one device array of a format; free it first unless another copy of the handle owns it.
template <class T>
static void release(T*& p, bool free_it) {
  if (p && free_it) (void)hipFree(p);
  p = nullptr;
}

// ---------------------------------------------------------------- SELL-64 construction
__global__ void k_sell_fill(const int32_t* __restrict__ ip, const int32_t* __restrict__ ij,
                            const double* __restrict__ ax, int64_t n, int64_t n_slices,
                            const int64_t* __restrict__ sp, const int32_t* __restrict__ perm,
                            int32_t* __restrict__ cols, double* __restrict__ vals) {
  const int64_t sl = blockIdx.x * 4ll + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (sl >= n_slices) return;
  const int64_t base = sp[sl];
  const int w = (int)((sp[sl + 1] - base) >> 6);
  const int64_t srow = sl * 64 + lane;
  const int64_t row = (perm && srow < n) ? perm[srow] : srow;
  const int a = row < n ? ip[row] : 0;
  const int len = row < n ? ip[row + 1] - a : 0;
  for (int k = 0; k < w; ++k) {
    const int64_t o = base + (int64_t)k * 64 + lane;
    cols[o] = k < len ? ij[a + k] : -1;
    vals[o] = k < len ? ax[a + k] : 0.0;
  }
}

static void drop_sell(mlamg_csr* A, bool free_it = true) {
  release(A->dict_code, free_it);
  release(A->dict_ptr, free_it);
  release(A->dict_off, free_it);
  release(A->dict_val, free_it);
  A->dict_n_off = A->dict_n_val = 0;
  release(A->sell_ptr, free_it);
  release(A->sell_col, free_it);
  release(A->sell_val, free_it);
  release(A->sell_perm, free_it);
  A->sell_sigma = 0;
  A->n_slices = 0;
  A->sell_elems = 0;
}

// Layout on the host from the row lengths: with sigma > 1 the rows of each window of sigma rows
// are ordered by decreasing length (stable), so a slice's rows have similar lengths and little
// padding (SELL-C-sigma); perm[k] = original row of sorted position k. Each row keeps its own
// entry order, so sums are unchanged; only which lane computes which row moves.
static int build_sell(mlamg_csr* A, hipStream_t s, int sigma) {
  drop_sell(A);
  const int64_t n = A->n_rows;
  const int64_t ns = (n + 63) / 64;
  std::vector<int32_t> ip(n + 1);
  MLAMG_HIP(hipMemcpyAsync(ip.data(), A->indptr, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost, s));
  MLAMG_HIP(hipStreamSynchronize(s));
  std::vector<int32_t> perm;
  if (sigma > 1) {
    perm.resize(n);
    for (int64_t i = 0; i < n; ++i) perm[i] = (int32_t)i;
    for (int64_t w0 = 0; w0 < n; w0 += sigma) {
      const int64_t w1 = std::min<int64_t>(n, w0 + sigma);
      std::stable_sort(perm.begin() + w0, perm.begin() + w1, [&](int32_t a, int32_t b) {
        return (ip[a + 1] - ip[a]) > (ip[b + 1] - ip[b]);
      });
    }
  }
  std::vector<int64_t> sp(ns + 1, 0);
  for (int64_t sl = 0; sl < ns; ++sl) {
    int32_t w = 0;
    for (int64_t k = sl * 64; k < std::min<int64_t>(n, sl * 64 + 64); ++k) {
      const int32_t r = perm.empty() ? (int32_t)k : perm[k];
      w = std::max(w, ip[r + 1] - ip[r]);
    }
    sp[sl + 1] = sp[sl] + 64ll * w;
  }
  const int64_t total = sp[ns];
  if (hipMalloc(&A->sell_ptr, sizeof(int64_t) * (ns + 1)) != hipSuccess ||
      hipMalloc(&A->sell_col, sizeof(int32_t) * std::max<int64_t>(total, 1)) != hipSuccess ||
      hipMalloc(&A->sell_val, sizeof(double) * std::max<int64_t>(total, 1)) != hipSuccess ||
      (!perm.empty() && hipMalloc(&A->sell_perm, sizeof(int32_t) * n) != hipSuccess)) {
    drop_sell(A);
    set_error("build_sell: out of device memory");
    return MLAMG_ENOMEM;
  }
  MLAMG_HIP(hipMemcpyAsync(A->sell_ptr, sp.data(), sizeof(int64_t) * (ns + 1), hipMemcpyHostToDevice, s));
  if (!perm.empty())
    MLAMG_HIP(hipMemcpyAsync(A->sell_perm, perm.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
  if (ns)
    hipLaunchKernelGGL(k_sell_fill, dim3((ns + 3) / 4), dim3(256), 0, s, A->indptr, A->indices,
                       A->data, n, ns, A->sell_ptr, A->sell_perm, A->sell_col, A->sell_val);
  MLAMG_HIP(hipGetLastError());
  MLAMG_HIP(hipStreamSynchronize(s));
  A->n_slices = ns;
  A->sell_elems = total;
  A->sell_sigma = std::max(sigma, 1);
  return MLAMG_OK;
}

// ---------------------------------------------------------------- dictionary construction
// Open-addressing tables of kDictSlots 64-bit keys; a slot holds kDictEmpty until claimed.
constexpr int kDictSlots = 1024;
constexpr unsigned long long kDictEmpty = ~0ull;

__device__ __forceinline__ int dict_slot(unsigned long long key, unsigned long long* tab,
                                         int32_t* count, bool insert) {
  unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 54);  // 10 bits
  for (int probe = 0; probe < kDictSlots; ++probe) {
    const unsigned sl = (h + probe) & (kDictSlots - 1);
    unsigned long long cur = tab[sl];
    if (cur == key) return (int)sl;
    if (cur == kDictEmpty) {
      if (!insert) return -1;
      cur = atomicCAS(&tab[sl], kDictEmpty, key);
      if (cur == kDictEmpty) {
        atomicAdd(count, 1);
        return (int)sl;
      }
      if (cur == key) return (int)sl;
    }
  }
  return -1;
}

// pass 0: insert every (offset, value) of the SELL copy; pass 1: encode with slot -> index maps
__global__ void k_dict_pass(const int64_t* __restrict__ sp, const int32_t* __restrict__ cols,
                            const double* __restrict__ vals, const int32_t* __restrict__ perm,
                            int64_t n, int64_t n_slices, int pass, unsigned long long* otab,
                            unsigned long long* vtab, int32_t* counts,
                            const int32_t* __restrict__ oidx, const int32_t* __restrict__ vidx,
                            const int64_t* __restrict__ dp, uint16_t* __restrict__ codes) {
  const int64_t sl = blockIdx.x * 4ll + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (sl >= n_slices) return;
  const int64_t base = sp[sl];
  const int w = (int)((sp[sl + 1] - base) >> 6);
  const int64_t srow = sl * 64 + lane;
  const int64_t row = (perm && srow < n) ? perm[srow] : srow;
  for (int k = 0; k < w; ++k) {
    const int64_t o = base + (int64_t)k * 64 + lane;
    const int32_t c = cols[o];
    if (pass == 0) {
      // stop as soon as the dictionaries are known to overflow
      if (((volatile int32_t*)counts)[0] > 255 || ((volatile int32_t*)counts)[1] > 256 ||
          ((volatile int32_t*)counts)[2] != 0)
        return;
      if (c < 0) continue;
      const unsigned long long okey = (unsigned long long)((int64_t)c - row + (int64_t(1) << 40));
      const unsigned long long vkey = (unsigned long long)__double_as_longlong(vals[o]);
      if (dict_slot(okey, otab, counts + 0, true) < 0 || vkey == kDictEmpty ||
          dict_slot(vkey, vtab, counts + 1, true) < 0)
        atomicAdd(counts + 2, 1);  // table full / unrepresentable: refuse the format
    } else {
      if (c < 0) continue;  // padding: the code array is pre-filled with 0x00FF
      const unsigned long long okey = (unsigned long long)((int64_t)c - row + (int64_t(1) << 40));
      const unsigned long long vkey = (unsigned long long)__double_as_longlong(vals[o]);
      const int so = dict_slot(okey, otab, counts, false), sv = dict_slot(vkey, vtab, counts, false);
      codes[dp[sl] + ((int64_t)(k >> 3) << 9) + lane * 8 + (k & 7)] =
          (uint16_t)(oidx[so] | (vidx[sv] << 8));
    }
  }
}

// SELL (natural order or sigma-sorted) re-coded with dictionaries; EUNSUPPORTED (the SELL
// copy dropped again) when the operator has more than 255 distinct offsets or 256 distinct values.
static int build_sell_dict(mlamg_csr* A, hipStream_t s, int sigma) {
  MLAMG_TRY(build_sell(A, s, sigma));
  const int64_t ns = A->n_slices;
  // packed code layout: each slice's rows padded to a multiple of 8 codes
  std::vector<int64_t> hsp(ns + 1), hdp(ns + 1, 0);
  MLAMG_HIP(hipMemcpyAsync(hsp.data(), A->sell_ptr, sizeof(int64_t) * (ns + 1),
                           hipMemcpyDeviceToHost, s));
  MLAMG_HIP(hipStreamSynchronize(s));
  for (int64_t sl = 0; sl < ns; ++sl) {
    const int64_t w = (hsp[sl + 1] - hsp[sl]) >> 6;
    hdp[sl + 1] = hdp[sl] + ((w + 7) / 8) * 512;
  }
  const int64_t n_codes = hdp[ns];
  unsigned long long *otab = nullptr, *vtab = nullptr;
  int32_t *counts = nullptr, *oidx = nullptr, *vidx = nullptr;
  int rc = MLAMG_OK;
  auto fail = [&](int code, const char* what) {
    if (rc == MLAMG_OK) {
      set_error(std::string("sell_dict: ") + what);
      rc = code;
    }
  };
  if (hipMalloc(&otab, sizeof(unsigned long long) * kDictSlots) != hipSuccess ||
      hipMalloc(&vtab, sizeof(unsigned long long) * kDictSlots) != hipSuccess ||
      hipMalloc(&counts, sizeof(int32_t) * 4) != hipSuccess ||
      hipMalloc(&oidx, sizeof(int32_t) * kDictSlots) != hipSuccess ||
      hipMalloc(&vidx, sizeof(int32_t) * kDictSlots) != hipSuccess ||
      hipMalloc(&A->dict_code, sizeof(uint16_t) * std::max<int64_t>(n_codes, 8)) != hipSuccess ||
      hipMalloc(&A->dict_ptr, sizeof(int64_t) * (ns + 1)) != hipSuccess ||
      hipMalloc(&A->dict_off, sizeof(int32_t) * 256) != hipSuccess ||
      hipMalloc(&A->dict_val, sizeof(double) * 256) != hipSuccess)
    fail(MLAMG_ENOMEM, "out of device memory");
  if (rc == MLAMG_OK &&
      (hipMemsetAsync(otab, 0xFF, sizeof(unsigned long long) * kDictSlots, s) != hipSuccess ||
       hipMemsetAsync(vtab, 0xFF, sizeof(unsigned long long) * kDictSlots, s) != hipSuccess ||
       hipMemsetAsync(counts, 0, sizeof(int32_t) * 4, s) != hipSuccess ||
       hipMemsetAsync(A->dict_off, 0, sizeof(int32_t) * 256, s) != hipSuccess ||
       hipMemsetAsync(A->dict_val, 0, sizeof(double) * 256, s) != hipSuccess ||
       hipMemsetD16Async((hipDeviceptr_t)A->dict_code, 0x00FF, (size_t)std::max<int64_t>(n_codes, 8),
                         s) != hipSuccess ||
       hipMemcpyAsync(A->dict_ptr, hdp.data(), sizeof(int64_t) * (ns + 1), hipMemcpyHostToDevice,
                      s) != hipSuccess))
    fail(MLAMG_EHIP, "memset");
  if (rc == MLAMG_OK && ns)
    hipLaunchKernelGGL(k_dict_pass, dim3((ns + 3) / 4), dim3(256), 0, s, A->sell_ptr, A->sell_col,
                       A->sell_val, A->sell_perm, A->n_rows, ns, 0, otab, vtab, counts, oidx,
                       vidx, A->dict_ptr, A->dict_code);
  std::vector<unsigned long long> ho(kDictSlots), hv(kDictSlots);
  int32_t hc[4] = {0, 0, 0, 0};
  if (rc == MLAMG_OK &&
      (hipGetLastError() != hipSuccess ||
       hipMemcpyAsync(ho.data(), otab, sizeof(unsigned long long) * kDictSlots,
                      hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipMemcpyAsync(hv.data(), vtab, sizeof(unsigned long long) * kDictSlots,
                      hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipMemcpyAsync(hc, counts, sizeof(hc), hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipStreamSynchronize(s) != hipSuccess))
    fail(MLAMG_EHIP, "dictionary scan");
  if (rc == MLAMG_OK && (hc[2] != 0 || hc[0] > 255 || hc[1] > 256))
    fail(MLAMG_EUNSUPPORTED, "more than 255 distinct column offsets or 256 distinct values");
  if (rc == MLAMG_OK) {
    // deterministic indices: offsets ascending, values by ascending bit pattern
    std::vector<std::pair<unsigned long long, int>> os, vs;
    for (int i = 0; i < kDictSlots; ++i) {
      if (ho[i] != kDictEmpty) os.push_back({ho[i], i});
      if (hv[i] != kDictEmpty) vs.push_back({hv[i], i});
    }
    std::sort(os.begin(), os.end());
    std::sort(vs.begin(), vs.end());
    std::vector<int32_t> hoi(kDictSlots, 0), hvi(kDictSlots, 0), offt(256, 0);
    std::vector<double> valt(256, 0.0);
    for (size_t k = 0; k < os.size(); ++k) {
      hoi[os[k].second] = (int32_t)k;
      offt[k] = (int32_t)((int64_t)os[k].first - (int64_t(1) << 40));
    }
    for (size_t k = 0; k < vs.size(); ++k) {
      hvi[vs[k].second] = (int32_t)k;
      std::memcpy(&valt[k], &vs[k].first, sizeof(double));
    }
    A->dict_n_off = (int32_t)os.size();
    A->dict_n_val = (int32_t)vs.size();
    if (hipMemcpyAsync(oidx, hoi.data(), sizeof(int32_t) * kDictSlots, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(vidx, hvi.data(), sizeof(int32_t) * kDictSlots, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(A->dict_off, offt.data(), sizeof(int32_t) * 256, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(A->dict_val, valt.data(), sizeof(double) * 256, hipMemcpyHostToDevice, s) != hipSuccess)
      fail(MLAMG_EHIP, "upload");
    if (rc == MLAMG_OK && ns)
      hipLaunchKernelGGL(k_dict_pass, dim3((ns + 3) / 4), dim3(256), 0, s, A->sell_ptr,
                         A->sell_col, A->sell_val, A->sell_perm, A->n_rows, ns, 1, otab, vtab,
                         counts, oidx, vidx, A->dict_ptr, A->dict_code);
    if (rc == MLAMG_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess))
      fail(MLAMG_EHIP, "encode");
  }
  for (void* p : {(void*)otab, (void*)vtab, (void*)counts, (void*)oidx, (void*)vidx})
    if (p) (void)hipFree(p);
  if (rc != MLAMG_OK) {
    drop_sell(A);
    return rc;
  }
  // the coded copy replaces the SELL arrays
  (void)hipFree(A->sell_col);
  (void)hipFree(A->sell_val);
  A->sell_col = nullptr;
  A->sell_val = nullptr;
  return MLAMG_OK;
}

// ---------------------------------------------------------------- sorted-format construction
__global__ void k_srt_keys(const int32_t* __restrict__ ip, const int32_t* __restrict__ ij,
                           const int32_t* __restrict__ blk, int cbits, uint64_t* __restrict__ key,
                           int32_t* __restrict__ idx) {
  const int b = blockIdx.x;
  const int a = ip[blk[b]], z = ip[blk[b + 1]];
  for (int e = a + (int)threadIdx.x; e < z; e += blockDim.x) {
    key[e] = ((uint64_t)b << cbits) | (uint32_t)ij[e];
    idx[e] = e;
  }
}

// One workgroup per block over its column-sorted entries: a single window [lo, lo + 2^20) if
// the columns fit, else split at the widest gap between consecutive columns into two windows
// (each must fit); otherwise the block is too wide and the format is refused.
__global__ __launch_bounds__(256) void k_srt_pack(const int32_t* __restrict__ ip,
                                                  const double* __restrict__ ax,
                                                  const int32_t* __restrict__ blk,
                                                  const uint64_t* __restrict__ key,
                                                  const int32_t* __restrict__ idx, uint64_t cmask,
                                                  int32_t* __restrict__ base,
                                                  uint32_t* __restrict__ pk,
                                                  double* __restrict__ av,
                                                  int32_t* __restrict__ too_wide) {
  __shared__ int64_t best[256];
  const int b = blockIdx.x;
  const int a = ip[blk[b]], z = ip[blk[b + 1]];
  const int m = z - a;
  if (m == 0) {
    if (threadIdx.x == 0) base[8 * b + 4] = base[8 * b + 5] = base[8 * b + 6] = 0;
    return;
  }
  auto col = [&](int e) { return (int64_t)(key[a + e] & cmask); };
  const int64_t span = int64_t(1) << (32 - kSrtPosBits);
  int split = m;
  if (col(m - 1) - col(0) >= span) {
    // argmax gap (gap << 32 | position, max picks the widest, ties the last)
    int64_t bv = -1;
    for (int e = 1 + (int)threadIdx.x; e < m; e += 256) {
      const int64_t g = ((col(e) - col(e - 1)) << 32) | e;
      bv = g > bv ? g : bv;
    }
    best[threadIdx.x] = bv;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o && best[threadIdx.x + o] > best[threadIdx.x])
        best[threadIdx.x] = best[threadIdx.x + o];
      __syncthreads();
    }
    split = (int)(best[0] & 0xffffffff);
    if (col(split - 1) - col(0) >= span || col(m - 1) - col(split) >= span) {
      if (threadIdx.x == 0) atomicAdd(too_wide, 1);
      return;
    }
  }
  const int lo = (int)col(0), hi = split < m ? (int)col(split) : lo;
  if (threadIdx.x == 0) {
    base[8 * b + 4] = lo;
    base[8 * b + 5] = hi;
    base[8 * b + 6] = split;
  }
  for (int e = (int)threadIdx.x; e < m; e += 256) {
    const int src = idx[a + e];
    const int c = (int)col(e) - (e < split ? lo : hi);
    pk[a + e] = ((uint32_t)c << kSrtPosBits) | (uint32_t)(src - a);
    av[a + e] = ax[src];
  }
}

__global__ void k_vdict_scan(const double* __restrict__ v, int64_t n, unsigned long long* vtab,
                             int32_t* counts) {
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    if (((volatile int32_t*)counts)[1] > 256 || ((volatile int32_t*)counts)[2] != 0) return;
    const unsigned long long key = (unsigned long long)__double_as_longlong(v[e]);
    if (key == kDictEmpty || dict_slot(key, vtab, counts + 1, true) < 0) atomicAdd(counts + 2, 1);
  }
}

__global__ void k_vdict_encode(const double* __restrict__ v, int64_t n, unsigned long long* vtab,
                               const int32_t* __restrict__ vidx, uint8_t* __restrict__ out) {
  const int64_t e = blockIdx.x * 256ll + threadIdx.x;
  if (e >= n) return;
  const unsigned long long key = (unsigned long long)__double_as_longlong(v[e]);
  out[e] = (uint8_t)vidx[dict_slot(key, vtab, nullptr, false)];
}

static void drop_vector(mlamg_csr* A, bool free_it = true) {
  A->vec_width = 0;
  release(A->vec_idx16, free_it);
}

__global__ void k_idx16(const int32_t* __restrict__ in, uint16_t* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint16_t)in[i];
}

// 16-bit column copies for the VECTOR format (n_cols <= 65536; env MLAMG_NO_IDX16 = A/B knob)
static int build_vec16(mlamg_csr* A, hipStream_t s) {
  release(A->vec_idx16, true);
  if (A->n_cols > 65536 || A->nnz == 0 || getenv("MLAMG_NO_IDX16")) return MLAMG_OK;
  uint16_t* d = nullptr;
  if (hipMalloc(&d, sizeof(uint16_t) * (size_t)A->nnz) != hipSuccess) {
    (void)hipGetLastError();
    return MLAMG_OK;  // optional copy: the 32-bit indices serve
  }
  hipLaunchKernelGGL(k_idx16, dim3((unsigned)((A->nnz + 255) / 256)), dim3(256), 0, s, A->indices,
                     d, A->nnz);
  MLAMG_HIP(hipGetLastError());
  A->vec_idx16 = d;
  return MLAMG_OK;
}

static void drop_long(mlamg_csr* A, bool free_it = true) {
  release(A->lg_tile, free_it);
  A->lg_nt = 0;
}

// Tiles of the "long" format: consecutive rows while the tile has <= kLongRows rows and
// <= kLongNnz nonzeros; a longer row is a tile of its own (streamed in chunks by the kernel).
static int build_long(mlamg_csr* A, hipStream_t s) {
  const int64_t n = A->n_rows;
  std::vector<int32_t> ip(n + 1);
  MLAMG_HIP(hipMemcpyAsync(ip.data(), A->indptr, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost,
                           s));
  MLAMG_HIP(hipStreamSynchronize(s));
  std::vector<int32_t> t(1, 0);
  for (int64_t r = 0; r < n;) {
    int64_t r1 = r, nz = 0;
    while (r1 < n && r1 - r < kLongRows && nz + (ip[r1 + 1] - ip[r1]) <= kLongNnz) {
      nz += ip[r1 + 1] - ip[r1];
      ++r1;
    }
    if (r1 == r) r1 = r + 1;
    t.push_back((int32_t)r1);
    r = r1;
  }
  int32_t* d = nullptr;
  MLAMG_HIP(hipMalloc(&d, sizeof(int32_t) * t.size()));
  if (hipMemcpyAsync(d, t.data(), sizeof(int32_t) * t.size(), hipMemcpyHostToDevice, s) !=
          hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    (void)hipFree(d);
    set_error("build_long: upload failed");
    return MLAMG_EHIP;
  }
  if (A->lg_tile) (void)hipFree(A->lg_tile);
  A->lg_tile = d;
  A->lg_nt = (int32_t)(t.size() - 1);
  return MLAMG_OK;
}

static void drop_sorted(mlamg_csr* A, bool free_it = true) {
  release(A->srt_blk, free_it);
  release(A->srt_base, free_it);
  release(A->srt_pk, free_it);
  release(A->srt_val, free_it);
  release(A->srt_vi, free_it);
  release(A->srt_vtab, free_it);
  release(A->srt_vc, free_it);
  release(A->srt_vblk, free_it);
  A->srt_vtab_n = 0;
  A->srt_nb = 0;
}

// Replace the sorted copy's fp64 values by one-byte indices into a table when the operator has
// at most 256 distinct values (bit patterns). Returns EUNSUPPORTED (nothing changed) otherwise.
static int sorted_value_dict(mlamg_csr* A, hipStream_t s) {
  const int64_t nnz = A->nnz;
  if (!A->srt_val || nnz == 0) return MLAMG_EUNSUPPORTED;
  unsigned long long* vtab = nullptr;
  int32_t *counts = nullptr, *vidx = nullptr;
  uint8_t* vi = nullptr;
  double* table = nullptr;
  int rc = MLAMG_OK;
  if (hipMalloc(&vtab, sizeof(unsigned long long) * kDictSlots) != hipSuccess ||
      hipMalloc(&counts, sizeof(int32_t) * 4) != hipSuccess ||
      hipMalloc(&vidx, sizeof(int32_t) * kDictSlots) != hipSuccess ||
      hipMemsetAsync(vtab, 0xFF, sizeof(unsigned long long) * kDictSlots, s) != hipSuccess ||
      hipMemsetAsync(counts, 0, sizeof(int32_t) * 4, s) != hipSuccess)
    rc = MLAMG_ENOMEM;
  std::vector<unsigned long long> hv(kDictSlots);
  int32_t hc[4] = {0, 0, 0, 0};
  if (rc == MLAMG_OK) {
    const int64_t nb = std::min<int64_t>((nnz + 255) / 256, 8192);
    hipLaunchKernelGGL(k_vdict_scan, dim3((unsigned)nb), dim3(256), 0, s, A->srt_val, nnz, vtab,
                       counts);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(hv.data(), vtab, sizeof(unsigned long long) * kDictSlots,
                       hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(hc, counts, sizeof(hc), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc = MLAMG_EHIP;
  }
  if (rc == MLAMG_OK && (hc[2] != 0 || hc[1] > 256)) rc = MLAMG_EUNSUPPORTED;
  if (rc == MLAMG_OK) {
    std::vector<std::pair<unsigned long long, int>> vs;
    for (int i = 0; i < kDictSlots; ++i)
      if (hv[i] != kDictEmpty) vs.push_back({hv[i], i});
    std::sort(vs.begin(), vs.end());
    std::vector<int32_t> hvi(kDictSlots, 0);
    std::vector<double> valt(256, 0.0);
    for (size_t k = 0; k < vs.size(); ++k) {
      hvi[vs[k].second] = (int32_t)k;
      std::memcpy(&valt[k], &vs[k].first, sizeof(double));
    }
    if (hipMalloc(&vi, (size_t)nnz) != hipSuccess || hipMalloc(&table, sizeof(double) * 256) != hipSuccess)
      rc = MLAMG_ENOMEM;
    if (rc == MLAMG_OK &&
        (hipMemcpyAsync(vidx, hvi.data(), sizeof(int32_t) * kDictSlots, hipMemcpyHostToDevice, s) != hipSuccess ||
         hipMemcpyAsync(table, valt.data(), sizeof(double) * 256, hipMemcpyHostToDevice, s) != hipSuccess))
      rc = MLAMG_EHIP;
    if (rc == MLAMG_OK) {
      hipLaunchKernelGGL(k_vdict_encode, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, s,
                         A->srt_val, nnz, vtab, vidx, vi);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) rc = MLAMG_EHIP;
    }
  }
  for (void* p : {(void*)vtab, (void*)counts, (void*)vidx})
    if (p) (void)hipFree(p);
  if (rc != MLAMG_OK) {
    if (vi) (void)hipFree(vi);
    if (table) (void)hipFree(table);
    return rc;
  }
  (void)hipFree(A->srt_val);
  A->srt_val = nullptr;
  A->srt_vi = vi;
  A->srt_vtab = table;
  return MLAMG_OK;
}

// ---------------------------------------------------------------- sorted-format block dictionaries
// Round 5, VERDICT r04 Next #3. A_1 of C4 holds 455 k distinct values among 39.7 M entries, but
// a global table of them is gathered: 64 lanes on up to 64 lines per wave-instruction, and the
// coded kernel ran 130-160 us against 90 us for the fp64 values (tools/vc_ab.py).
// Each 4,096-entry block holds ~1,700 distinct values, so each block gets its own dictionary:
// read as one contiguous stream, staged in the LDS the products use later, and looked up there.
__global__ void k_vc_bits(const double* __restrict__ v, int64_t n, uint64_t* __restrict__ k,
                          int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    k[i] = __double_as_longlong(v[i]);
    idx[i] = (int32_t)i;
  }
}
// run heads of the block-sorted values: a new distinct value, or a block's first entry
__global__ void k_bd_heads(const uint64_t* __restrict__ k, int64_t n,
                           int32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) head[i] = (i == 0 || k[i] != k[i - 1]) ? 1 : 0;
}
__global__ void k_bd_block_heads(const int32_t* __restrict__ meta, int nb,
                                 int32_t* __restrict__ head) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < nb && meta[8 * b + 3] > 0) head[meta[8 * b + 2]] = 1;
}
// per block: its dictionary [off, off + size) of the table and each entry's code; the table
// entry of every run head
__global__ __launch_bounds__(256) void k_bd_encode(const int32_t* __restrict__ meta,
                                                   const uint64_t* __restrict__ k,
                                                   const int32_t* __restrict__ idx,
                                                   const int32_t* __restrict__ head,
                                                   const int32_t* __restrict__ scan,
                                                   uint16_t* __restrict__ code,
                                                   double* __restrict__ tab,
                                                   int32_t* __restrict__ vblk) {
  const int b = blockIdx.x;
  const int e0 = meta[8 * b + 2], ne = meta[8 * b + 3];
  const int off = scan[e0];
  if (threadIdx.x == 0) {
    vblk[2 * b] = off;
    vblk[2 * b + 1] = scan[e0 + ne] - off;
  }
  for (int e = threadIdx.x; e < ne; e += 256) {
    const int g = e0 + e;
    const int id = scan[g] + head[g] - 1;  // the distinct value's index in the table
    code[idx[g]] = (uint16_t)(id - off);
    if (head[g]) tab[id] = __longlong_as_double(k[g]);
  }
}

// Replace the sorted copy's fp64 values by per-block dictionaries and two-byte codes (above).
// EUNSUPPORTED (nothing changed) when the dictionaries would not save bytes: more than half of
// the entries distinct within their blocks.
static int sorted_block_dict(mlamg_csr* A, const std::vector<int32_t>& meta, hipStream_t s) {
  const int64_t nnz = A->nnz;
  const int nb = A->srt_nb;
  if (!A->srt_val || nnz == 0 || nb == 0 || nnz >= (int64_t(1) << 31)) return MLAMG_EUNSUPPORTED;
  uint64_t *k0 = nullptr, *k1 = nullptr;
  int32_t *i0 = nullptr, *i1 = nullptr, *head = nullptr, *scan = nullptr, *offs = nullptr;
  int32_t *dmeta = nullptr, *vblk = nullptr;
  void* tmp = nullptr;
  uint16_t* code = nullptr;
  double* tab = nullptr;
  int rc = MLAMG_OK;
  auto ok = [&](hipError_t e) {
    if (e != hipSuccess && rc == MLAMG_OK) {
      set_error(std::string("sorted block dictionaries: ") + hipGetErrorString(e));
      rc = MLAMG_EHIP;
    }
    return rc == MLAMG_OK;
  };
  const unsigned g = (unsigned)((nnz + 255) / 256);
  std::vector<int32_t> ho(nb + 1);
  for (int b = 0; b < nb; ++b) ho[b] = meta[8 * b + 2];
  ho[nb] = meta[8 * (nb - 1) + 2] + meta[8 * (nb - 1) + 3];
  int32_t total = 0;
  if (ok(hipMalloc(&k0, sizeof(uint64_t) * nnz)) && ok(hipMalloc(&k1, sizeof(uint64_t) * nnz)) &&
      ok(hipMalloc(&i0, sizeof(int32_t) * nnz)) && ok(hipMalloc(&i1, sizeof(int32_t) * nnz)) &&
      ok(hipMalloc(&head, sizeof(int32_t) * nnz)) &&
      ok(hipMalloc(&scan, sizeof(int32_t) * (nnz + 1))) &&
      ok(hipMalloc(&offs, sizeof(int32_t) * (nb + 1))) &&
      ok(hipMalloc(&dmeta, sizeof(int32_t) * 8 * nb)) &&
      ok(hipMemcpyAsync(offs, ho.data(), sizeof(int32_t) * (nb + 1), hipMemcpyHostToDevice, s)) &&
      ok(hipMemcpyAsync(dmeta, meta.data(), sizeof(int32_t) * 8 * nb, hipMemcpyHostToDevice, s))) {
    hipLaunchKernelGGL(k_vc_bits, dim3(g), dim3(256), 0, s, A->srt_val, nnz, k0, i0);
    ok(hipGetLastError());
    size_t tb = 0;
    ok(rocprim::segmented_radix_sort_pairs(nullptr, tb, k0, k1, i0, i1, (unsigned)nnz,
                                           (unsigned)nb, offs, offs + 1, 0, 64, s));
    if (ok(hipMalloc(&tmp, tb + 16)) &&
        ok(rocprim::segmented_radix_sort_pairs(tmp, tb, k0, k1, i0, i1, (unsigned)nnz,
                                               (unsigned)nb, offs, offs + 1, 0, 64, s))) {
      hipLaunchKernelGGL(k_bd_heads, dim3(g), dim3(256), 0, s, k1, nnz, head);
      hipLaunchKernelGGL(k_bd_block_heads, dim3((nb + 255) / 256), dim3(256), 0, s, dmeta, nb,
                         head);
      ok(hipGetLastError());
      if (rc == MLAMG_OK) rc = exclusive_scan_i32(head, scan, nnz, s);
      if (rc == MLAMG_OK) {
        ok(hipMemcpyAsync(&total, scan + nnz, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        ok(hipStreamSynchronize(s));
      }
    }
  }
  if (rc == MLAMG_OK && 2 * (int64_t)total > nnz) {
    set_error("sorted block dictionaries: more than half of the entries distinct per block");
    rc = MLAMG_EUNSUPPORTED;
  }
  if (rc == MLAMG_OK && ok(hipMalloc(&code, sizeof(uint16_t) * nnz)) &&
      ok(hipMalloc(&tab, sizeof(double) * std::max<int32_t>(total, 1))) &&
      ok(hipMalloc(&vblk, sizeof(int32_t) * 2 * nb))) {
    hipLaunchKernelGGL(k_bd_encode, dim3(nb), dim3(256), 0, s, dmeta, k1, i1, head, scan, code,
                       tab, vblk);
    ok(hipGetLastError());
    ok(hipStreamSynchronize(s));
  }
  for (void* q : {(void*)k0, (void*)k1, (void*)i0, (void*)i1, (void*)head, (void*)scan,
                  (void*)offs, (void*)dmeta, tmp})
    if (q) (void)hipFree(q);
  if (rc != MLAMG_OK) {
    for (void* q : {(void*)code, (void*)tab, (void*)vblk})
      if (q) (void)hipFree(q);
    return rc;
  }
  (void)hipFree(A->srt_val);
  A->srt_val = nullptr;
  A->srt_vc = code;
  A->srt_vtab = tab;
  A->srt_vblk = vblk;
  A->srt_vtab_n = total;
  return MLAMG_OK;
}

// Fixed-stride layout of the sorted copy: block b's entries at [b * kSrtNnz, (b + 1) * kSrtNnz),
// padded with `pad` (kNone codes, zero values): the kernel's entry loads then need no block
// record (e0, ne) and issue at launch, in parallel with the record load, instead of one memory
// round trip after it.
template <class T>
__global__ __launch_bounds__(256) void k_srt_pad(const T* __restrict__ src, T* __restrict__ dst,
                                                 const int32_t* __restrict__ meta, T pad) {
  const int b = blockIdx.x;
  const int e0 = meta[8 * b + 2], ne = meta[8 * b + 3];
  T* d = dst + (size_t)b * kSrtNnz;
  for (int e = threadIdx.x; e < kSrtNnz; e += 256) d[e] = e < ne ? src[e0 + e] : pad;
}

template <class T>
static int pad_stream(T** arr, int nb, const int32_t* meta, T pad, hipStream_t s) {
  T* d = nullptr;
  MLAMG_HIP(hipMalloc(&d, sizeof(T) * (size_t)kSrtNnz * std::max(nb, 1)));
  if (nb > 0) {
    hipLaunchKernelGGL((k_srt_pad<T>), dim3(nb), dim3(256), 0, s, *arr, d, meta, pad);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
      (void)hipFree(d);
      set_error("sorted format: padding pass failed");
      return MLAMG_EHIP;
    }
  }
  (void)hipFree(*arr);
  *arr = d;
  return MLAMG_OK;
}

// Row blocks of <= kSrtRows rows / <= kSrtNnz nonzeros; inside each, entries radix-sorted by
// (block, column) (stable, so equal columns keep CSR order; any order would give the same bits).
// EUNSUPPORTED (A unchanged) if a row is longer than kSrtNnz or a block's columns do not fit
// two windows of 2^20.
static int build_sorted(mlamg_csr* A, hipStream_t s, int value_mode = 0) {
  drop_sorted(A);
  const int64_t n = A->n_rows, nnz = A->nnz;
  if (A->n_cols >= (int64_t(1) << 28)) {  // k_sorted's x offsets are 32-bit byte offsets
    set_error("sorted format: more than 2^28 columns");
    return MLAMG_EUNSUPPORTED;
  }
  std::vector<int32_t> ip(n + 1);
  MLAMG_HIP(hipMemcpyAsync(ip.data(), A->indptr, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost, s));
  MLAMG_HIP(hipStreamSynchronize(s));
  std::vector<int32_t> blk{0};
  for (int64_t r = 0; r < n;) {
    int64_t e = r;
    while (e < n && e - r < kSrtRows && ip[e + 1] - ip[r] <= kSrtNnz) ++e;
    if (e == r) {
      set_error("sorted format: a row has more than 4096 nonzeros");
      return MLAMG_EUNSUPPORTED;
    }
    blk.push_back((int32_t)e);
    r = e;
  }
  const int nb = (int)blk.size() - 1;
  int cbits = 1;
  while ((int64_t(1) << cbits) < std::max<int64_t>(A->n_cols, 2)) ++cbits;
  int bbits = 1;
  while ((int64_t(1) << bbits) < std::max(nb, 2)) ++bbits;
  MLAMG_REQUIRE(cbits + bbits <= 64, "sorted format: key does not fit 64 bits");
  uint64_t *k0 = nullptr, *k1 = nullptr;
  int32_t *i0 = nullptr, *i1 = nullptr, *wide = nullptr;
  void* tmp = nullptr;
  int rc = MLAMG_OK;
  auto fail = [&](const char* what) {
    if (rc == MLAMG_OK) {
      set_error(std::string("sorted format: ") + what);
      rc = MLAMG_ENOMEM;
    }
  };
  const size_t m = (size_t)std::max<int64_t>(nnz, 1);
  if (hipMalloc(&A->srt_blk, sizeof(int32_t) * (nb + 1)) != hipSuccess ||
      hipMalloc(&A->srt_base, sizeof(int32_t) * 8 * std::max(nb, 1)) != hipSuccess ||
      hipMalloc(&A->srt_pk, sizeof(uint32_t) * m) != hipSuccess ||
      hipMalloc(&A->srt_val, sizeof(double) * m) != hipSuccess ||
      hipMalloc(&k0, sizeof(uint64_t) * m) != hipSuccess ||
      hipMalloc(&k1, sizeof(uint64_t) * m) != hipSuccess ||
      hipMalloc(&i0, sizeof(int32_t) * m) != hipSuccess ||
      hipMalloc(&i1, sizeof(int32_t) * m) != hipSuccess ||
      hipMalloc(&wide, sizeof(int32_t)) != hipSuccess)
    fail("out of device memory");
  // per block {r0, r1, e0, nnz, lo, hi, split, 0}; k_srt_pack fills the column windows
  std::vector<int32_t> meta(8 * (size_t)std::max(nb, 1), 0);
  for (int b = 0; b < nb; ++b) {
    meta[8 * b] = blk[b];
    meta[8 * b + 1] = blk[b + 1];
    meta[8 * b + 2] = ip[blk[b]];
    meta[8 * b + 3] = ip[blk[b + 1]] - ip[blk[b]];
  }
  if (rc == MLAMG_OK &&
      (hipMemcpyAsync(A->srt_blk, blk.data(), sizeof(int32_t) * (nb + 1), hipMemcpyHostToDevice,
                      s) != hipSuccess ||
       hipMemcpyAsync(A->srt_base, meta.data(), sizeof(int32_t) * meta.size(),
                      hipMemcpyHostToDevice, s) != hipSuccess ||
       hipMemsetAsync(wide, 0, sizeof(int32_t), s) != hipSuccess))
    fail("upload");
  if (rc == MLAMG_OK && nb > 0 && nnz > 0) {
    hipLaunchKernelGGL(k_srt_keys, dim3(nb), dim3(256), 0, s, A->indptr, A->indices, A->srt_blk,
                       cbits, k0, i0);
    size_t tb = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, k0, k1, i0, i1, (size_t)nnz, 0,
                                             cbits + bbits, s);
    if (e == hipSuccess) e = hipMalloc(&tmp, tb + 16);
    if (e == hipSuccess)
      e = rocprim::radix_sort_pairs(tmp, tb, k0, k1, i0, i1, (size_t)nnz, 0, cbits + bbits, s);
    if (e != hipSuccess) fail("radix sort");
    if (rc == MLAMG_OK)
      hipLaunchKernelGGL(k_srt_pack, dim3(nb), dim3(256), 0, s, A->indptr, A->data, A->srt_blk, k1,
                         i1, (uint64_t(1) << cbits) - 1, A->srt_base, A->srt_pk, A->srt_val, wide);
  }
  int32_t too_wide = 0;
  if (rc == MLAMG_OK &&
      (hipGetLastError() != hipSuccess ||
       hipMemcpyAsync(&too_wide, wide, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipStreamSynchronize(s) != hipSuccess))
    fail("kernel launch");
  for (void* p : {(void*)k0, (void*)k1, (void*)i0, (void*)i1, (void*)wide, tmp})
    if (p) (void)hipFree(p);
  if (rc == MLAMG_OK && too_wide) {
    set_error("sorted format: a block's columns do not fit two windows of 2^20");
    rc = MLAMG_EUNSUPPORTED;
  }
  if (rc != MLAMG_OK) {
    drop_sorted(A);
    return rc;
  }
  A->srt_nb = nb;
  (void)sorted_value_dict(A, s);  // optional: keeps the fp64 values when it does not apply
  if (value_mode == 2) {
    // value codes asked for: refused (EUNSUPPORTED, the format dropped) where they do not apply
    // — including <= 256 values, where the one-byte dictionary (format 'sorted') is smaller
    rc = A->srt_vi ? MLAMG_EUNSUPPORTED : sorted_block_dict(A, meta, s);
    if (rc != MLAMG_OK) {
      drop_sorted(A);
      return rc;
    }
  }
  rc = pad_stream<uint32_t>(&A->srt_pk, nb, A->srt_base, 0xffffffffu, s);
  if (rc == MLAMG_OK)
    rc = A->srt_vi   ? pad_stream<uint8_t>(&A->srt_vi, nb, A->srt_base, (uint8_t)0, s)
         : A->srt_vc ? pad_stream<uint16_t>(&A->srt_vc, nb, A->srt_base, (uint16_t)0, s)
                     : pad_stream<double>(&A->srt_val, nb, A->srt_base, 0.0, s);
  if (rc != MLAMG_OK) drop_sorted(A);
  return rc;
}

// ---------------------------------------------------------------- row-pair pattern construction
// A pair's key: a 64-bit hash of both rows' lengths and (col - row, value bits) sequences. Pairs
// are inserted into an open-addressing table (<= 255 keys, else refused) with the smallest pair
// of each key as its representative; the host orders patterns by representative, reads their
// rows and merges them by offset (or, for rows not in ascending column order, by the shortest
// merge that keeps each row's stored order), and k_rp_assign then
// checks every pair against its pattern entry by entry (a hash collision makes the format
// refuse, it never changes a result).
__device__ __forceinline__ unsigned long long rp_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long rp_row_key(const int32_t* __restrict__ ip,
                                                         const int32_t* __restrict__ ij,
                                                         const double* __restrict__ ax,
                                                         int64_t row, unsigned long long h) {
  const int a = ip[row], b = ip[row + 1];
  h = rp_mix(h ^ (0x9E3779B97F4A7C15ull + (unsigned long long)(b - a)));
  for (int e = a; e < b; ++e) {
    h = rp_mix(h ^ (unsigned long long)(uint32_t)(ij[e] - (int32_t)row));
    h = rp_mix(h ^ (unsigned long long)__double_as_longlong(ax[e]));
  }
  return h;
}

// "wide" pair: every 16-byte load x[col0 .. col0+1] of the kernel's wide path is in range, i.e.
// row 2i's columns are <= n_cols - 2 and row 2i+1's >= 1 (false only at the matrix edges)
__device__ __forceinline__ bool rp_pair_wide(const int32_t* __restrict__ ip,
                                             const int32_t* __restrict__ ij, int64_t n,
                                             int64_t n_cols, int64_t pr) {
  if (2 * pr + 1 >= n) return false;
  for (int e = ip[2 * pr]; e < ip[2 * pr + 1]; ++e)
    if (ij[e] > n_cols - 2) return false;
  for (int e = ip[2 * pr + 1]; e < ip[2 * pr + 2]; ++e)
    if (ij[e] < 1) return false;
  return true;
}

__device__ __forceinline__ unsigned long long rp_pair_key(const int32_t* __restrict__ ip,
                                                          const int32_t* __restrict__ ij,
                                                          const double* __restrict__ ax,
                                                          int64_t n, int64_t n_cols, int64_t pr) {
  unsigned long long h = rp_row_key(ip, ij, ax, 2 * pr, 0x243F6A8885A308D3ull);
  h = 2 * pr + 1 < n ? rp_row_key(ip, ij, ax, 2 * pr + 1, h) : rp_mix(h ^ 0xA5A5A5A5ull);
  h = rp_mix(h ^ (rp_pair_wide(ip, ij, n, n_cols, pr) ? 0x1234567ull : 0x7654321ull));
  return h == kDictEmpty ? 0x5DEECE66Dull : h;
}

__global__ void k_rp_insert(const int32_t* __restrict__ ip, const int32_t* __restrict__ ij,
                            const double* __restrict__ ax, int64_t n, int64_t n_cols,
                            int64_t n_pairs, unsigned long long* tab, int32_t* rep,
                            int32_t* counts) {
  const int64_t pr = blockIdx.x * 256ll + threadIdx.x;
  if (pr >= n_pairs) return;
  if (((volatile int32_t*)counts)[0] > 255 || ((volatile int32_t*)counts)[2] != 0) return;
  const int sl = dict_slot(rp_pair_key(ip, ij, ax, n, n_cols, pr), tab, counts, true);
  if (sl < 0) {
    atomicAdd(counts + 2, 1);
    return;
  }
  if ((int32_t)pr < ((volatile int32_t*)rep)[sl]) atomicMin(rep + sl, (int32_t)pr);
}

// does row `row` consist exactly of the pattern entries flagged `bit`, in order? (pat_of[4k] =
// offset, pat_of[4k+3] = flags; pat_vv[2k + (bit == 2)] = the row's value)
__device__ __forceinline__ bool rp_row_matches(const int32_t* __restrict__ ip,
                                               const int32_t* __restrict__ ij,
                                               const double* __restrict__ ax, int64_t row,
                                               int pa, int pb, int bit,
                                               const int32_t* __restrict__ pat_of,
                                               const double* __restrict__ pat_vv) {
  int e = ip[row];
  const int eb = ip[row + 1];
  for (int k = pa; k < pb; ++k) {
    if (!(pat_of[4 * k + 3] & bit)) continue;  // bit 2 (wide) is not a row flag
    if (e >= eb || ij[e] - (int32_t)row != pat_of[4 * k] ||
        __double_as_longlong(ax[e]) != __double_as_longlong(pat_vv[2 * k + (bit == 2)]))
      return false;
    ++e;
  }
  return e == eb;
}

__global__ void k_rp_assign(const int32_t* __restrict__ ip, const int32_t* __restrict__ ij,
                            const double* __restrict__ ax, int64_t n, int64_t n_cols,
                            int64_t n_pairs, unsigned long long* tab,
                            const int32_t* __restrict__ slot_pid,
                            const int32_t* __restrict__ pat_ptr, const int32_t* __restrict__ pat_of,
                            const double* __restrict__ pat_vv, uint8_t* __restrict__ pid,
                            int32_t* bad) {
  const int64_t pr = blockIdx.x * 256ll + threadIdx.x;
  if (pr >= n_pairs) return;
  const int sl = dict_slot(rp_pair_key(ip, ij, ax, n, n_cols, pr), tab, nullptr, false);
  bool ok = sl >= 0;
  const int p = ok ? slot_pid[sl] : 0;
  if (ok) {
    const int pa = pat_ptr[p], pb = pat_ptr[p + 1];
    // the kernel takes the wide path on the first entry's bit 2: it must be this pair's own
    const bool wide_ok =
        pb == pa || ((pat_of[4 * pa + 3] & 4) != 0) == rp_pair_wide(ip, ij, n, n_cols, pr);
    ok = wide_ok && rp_row_matches(ip, ij, ax, 2 * pr, pa, pb, 1, pat_of, pat_vv);
    if (ok && 2 * pr + 1 < n)
      ok = rp_row_matches(ip, ij, ax, 2 * pr + 1, pa, pb, 2, pat_of, pat_vv);
    if (ok && 2 * pr + 1 >= n)  // the last pair of an odd n has no row 2i+1 entries
      for (int k = pa; k < pb; ++k) ok = ok && !(pat_of[4 * k + 3] & 2);
  }
  if (!ok) atomicAdd(bad, 1);
  pid[pr] = (uint8_t)p;
}

static void drop_rowpat(mlamg_csr* A, bool free_it = true) {
  release(A->rp_pid, free_it);
  release(A->rp_ptr, free_it);
  release(A->rp_off, free_it);
  release(A->rp_val, free_it);
  release(A->rp_dinv, free_it);
  release(A->rp_slot, free_it);
  release(A->rp_msk, free_it);
  A->rp_dinv_att = nullptr;
  A->rp_uni = RpUni{};
  A->rp_win = RpWin{};
  A->rp_mF = 0;
  A->rp_rep.clear();
  A->rp_n_pat = A->rp_n_ent = 0;
}

// EUNSUPPORTED (A unchanged) past 255 distinct pair patterns or kRpMaxEnt pattern entries.
static int build_rowpat(mlamg_csr* A, hipStream_t s) {
  const int64_t n = A->n_rows;
  const int64_t n_pairs = (n + 1) / 2;
  MLAMG_REQUIRE(n < (int64_t(1) << 31) - 1, "rowpat: more than 2^31 - 2 rows");
  if (A->n_cols >= (int64_t(1) << 29)) {  // x is addressed by 32-bit buffer byte offsets
    set_error("rowpat: more than 2^29 columns");
    return MLAMG_EUNSUPPORTED;
  }
  unsigned long long* tab = nullptr;
  int32_t *rep = nullptr, *counts = nullptr, *slot_pid = nullptr;
  uint8_t* pid = nullptr;
  int32_t *pptr = nullptr, *poff = nullptr;
  double* pval = nullptr;
  int rc = MLAMG_OK;
  auto fail = [&](int code, const std::string& what) {
    if (rc == MLAMG_OK) {
      set_error("rowpat: " + what);
      rc = code;
    }
  };
  if (hipMalloc(&tab, sizeof(unsigned long long) * kDictSlots) != hipSuccess ||
      hipMalloc(&rep, sizeof(int32_t) * kDictSlots) != hipSuccess ||
      hipMalloc(&counts, sizeof(int32_t) * 4) != hipSuccess ||
      hipMalloc(&slot_pid, sizeof(int32_t) * kDictSlots) != hipSuccess ||
      hipMalloc(&pid, std::max<int64_t>(n_pairs, 1)) != hipSuccess ||
      hipMalloc(&pptr, sizeof(int32_t) * 257) != hipSuccess)
    fail(MLAMG_ENOMEM, "out of device memory");
  if (rc == MLAMG_OK &&
      (hipMemsetAsync(tab, 0xFF, sizeof(unsigned long long) * kDictSlots, s) != hipSuccess ||
       hipMemsetAsync(rep, 0x7F, sizeof(int32_t) * kDictSlots, s) != hipSuccess ||
       hipMemsetAsync(counts, 0, sizeof(int32_t) * 4, s) != hipSuccess))
    fail(MLAMG_EHIP, "memset");
  const unsigned nb = (unsigned)((n_pairs + 255) / 256);
  if (rc == MLAMG_OK && n_pairs)
    hipLaunchKernelGGL(k_rp_insert, dim3(nb), dim3(256), 0, s, A->indptr, A->indices, A->data, n,
                       A->n_cols, n_pairs, tab, rep, counts);
  std::vector<unsigned long long> ht(kDictSlots);
  std::vector<int32_t> hrep(kDictSlots);
  int32_t hc[4] = {0, 0, 0, 0};
  if (rc == MLAMG_OK &&
      (hipGetLastError() != hipSuccess ||
       hipMemcpyAsync(ht.data(), tab, sizeof(unsigned long long) * kDictSlots,
                      hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipMemcpyAsync(hrep.data(), rep, sizeof(int32_t) * kDictSlots, hipMemcpyDeviceToHost,
                      s) != hipSuccess ||
       hipMemcpyAsync(hc, counts, sizeof(hc), hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipStreamSynchronize(s) != hipSuccess))
    fail(MLAMG_EHIP, "pattern scan");
  if (rc == MLAMG_OK && (hc[2] != 0 || hc[0] > 255))
    fail(MLAMG_EUNSUPPORTED, "more than 255 distinct row-pair patterns");
  std::vector<int32_t> hptr(257, 0), hoff, reps;
  RpWin win{};
  RpUni uni{};
  std::vector<uint16_t> hmsk;
  int kstep = 8;
  std::vector<double> hv0, hv1;
  std::vector<uint8_t> hfl;
  int n_pat = 0;
  if (rc == MLAMG_OK) {
    // patterns in order of first occurrence: deterministic ids
    std::vector<std::pair<int32_t, int>> pats;
    for (int i = 0; i < kDictSlots; ++i)
      if (ht[i] != kDictEmpty) pats.push_back({hrep[i], i});
    std::sort(pats.begin(), pats.end());
    n_pat = (int)pats.size();
    std::vector<int32_t> hslot(kDictSlots, 0);
    for (auto& pk : pats) reps.push_back(pk.first);
    auto fetch_row = [&](int64_t row, std::vector<int32_t>& off, std::vector<double>& val) {
      off.clear();
      val.clear();
      if (row >= n) return true;
      int32_t ab[2];
      if (hipMemcpy(ab, A->indptr + row, sizeof(ab), hipMemcpyDeviceToHost) != hipSuccess)
        return false;
      const int len = ab[1] - ab[0];
      off.resize(len);
      val.resize(len);
      if (len && (hipMemcpy(off.data(), A->indices + ab[0], sizeof(int32_t) * len,
                            hipMemcpyDeviceToHost) != hipSuccess ||
                  hipMemcpy(val.data(), A->data + ab[0], sizeof(double) * len,
                            hipMemcpyDeviceToHost) != hipSuccess))
        return false;
      for (auto& c : off) c -= (int32_t)row;
      return true;
    };
    std::vector<int32_t> o0, o1;
    std::vector<double> w0, w1;
    struct Ent {
      int32_t off;
      double v0, v1;
      uint8_t fl;
    };
    std::vector<std::vector<Ent>> pent(pats.size());
    std::vector<bool> pwide(pats.size(), false);
    bool all_sorted = true;
    size_t maxlen = 0;
    for (size_t k = 0; k < pats.size() && rc == MLAMG_OK; ++k) {
      hslot[pats[k].second] = (int32_t)k;
      const int64_t r0 = 2 * (int64_t)pats[k].first;
      if (!fetch_row(r0, o0, w0) || !fetch_row(r0 + 1, o1, w1)) {
        fail(MLAMG_EHIP, "pattern fetch");
        break;
      }
      bool sorted_rows = true;
      for (auto* o : {&o0, &o1})
        for (size_t e = 1; e < o->size(); ++e) sorted_rows = sorted_rows && (*o)[e] > (*o)[e - 1];
      all_sorted = all_sorted && sorted_rows;
      // wide (see rp_pair_wide): the same rule on the representative pair
      bool wide = r0 + 1 < n;
      for (int32_t o : o0) wide = wide && r0 + o <= A->n_cols - 2;
      for (int32_t o : o1) wide = wide && r0 + 1 + o >= 1;
      auto& pe = pent[k];
      auto emit = [&](bool t0, bool t1, size_t i, size_t j) {
        pe.push_back({t0 ? o0[i] : o1[j], t0 ? w0[i] : 0.0, t1 ? w1[j] : 0.0,
                      (uint8_t)((t0 ? 1 : 0) | (t1 ? 2 : 0) | (wide ? 4 : 0))});
      };
      if (sorted_rows) {
        // merge the two rows by offset (each row keeps its stored = ascending order)
        size_t i = 0, j = 0;
        while (i < o0.size() || j < o1.size()) {
          const bool t0 = i < o0.size() && (j >= o1.size() || o0[i] <= o1[j]);
          const bool t1 = j < o1.size() && (i >= o0.size() || o1[j] <= o0[i]);
          emit(t0, t1, i, j);
          i += t0;
          j += t1;
        }
      } else {
        // rows in stored but not ascending column order (a partitioned operator whose ghost
        // columns follow the owned ones, csrc/dhier.hip): the shortest merge that keeps each
        // row's stored order, sharing one 16-byte load where both rows have the same offset
        // (longest common subsequence of the two offset sequences)
        const size_t a = o0.size(), b = o1.size();
        std::vector<int32_t> L((a + 1) * (b + 1), 0);  // L[i][j] = LCS of o0[i:], o1[j:]
        for (size_t i = a; i-- > 0;)
          for (size_t j = b; j-- > 0;)
            L[i * (b + 1) + j] = o0[i] == o1[j] ? 1 + L[(i + 1) * (b + 1) + j + 1]
                                                : std::max(L[(i + 1) * (b + 1) + j],
                                                           L[i * (b + 1) + j + 1]);
        size_t i = 0, j = 0;
        while (i < a || j < b) {
          if (i < a && j < b && o0[i] == o1[j] &&
              L[i * (b + 1) + j] == 1 + L[(i + 1) * (b + 1) + j + 1]) {
            emit(true, true, i++, j++);
          } else if (j >= b || (i < a && L[(i + 1) * (b + 1) + j] >= L[i * (b + 1) + j + 1])) {
            emit(true, false, i++, j);
          } else {
            emit(false, true, i, j++);
          }
        }
      }
      pwide[k] = wide;
      maxlen = std::max(maxlen, pe.size());
    }
    // uniform form (k_rowpat_uni): every entry one of <= kRpUniMax offsets with one value per
    // (offset, row parity), rows in ascending column order (then each row sums in slot order)
    const char* uni_ev = std::getenv("MLAMG_RP_UNI");
    auto try_uni = [&](const std::vector<std::vector<Ent>>& P, bool sorted, RpUni& u,
                       std::vector<uint16_t>& msk) {
      u = RpUni{};
      bool ok = sorted && !(uni_ev && uni_ev[0] == '0') && n_pat <= 255;
      std::vector<int32_t> offs;
      for (auto& pe : P)
        for (auto& en : pe)
          if (en.fl & 3) offs.push_back(en.off);
      std::sort(offs.begin(), offs.end());
      offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
      ok = ok && !offs.empty() && offs.size() <= (size_t)kRpUniMax;
      bool set0[kRpUniMax] = {}, set1[kRpUniMax] = {};
      msk.assign(P.size(), 0);
      for (size_t k = 0; ok && k < P.size(); ++k)
        for (auto& en : P[k]) {
          if (!(en.fl & 3)) continue;
          const int q = (int)(std::lower_bound(offs.begin(), offs.end(), en.off) - offs.begin());
          auto same = [](double a, double b) {
            return __builtin_bit_cast(uint64_t, a) == __builtin_bit_cast(uint64_t, b);
          };
          if (en.fl & 1) {
            if (!set0[q]) u.v0[q] = en.v0;
            ok = ok && same(u.v0[q], en.v0);
            set0[q] = true;
            msk[k] |= (uint16_t)(1u << q);
          }
          if (en.fl & 2) {
            if (!set1[q]) u.v1[q] = en.v1;
            ok = ok && same(u.v1[q], en.v1);
            set1[q] = true;
            msk[k] |= (uint16_t)(1u << (q + 8));
          }
        }
      int halo = 2, nfar = 0;
      for (size_t q = 0; ok && q < offs.size(); ++q) {
        const int32_t o = offs[q];
        int kd;
        if (o == -1) kd = 1;
        else if (o == 1) kd = 2;
        else if ((o & 1) == 0 && std::abs(o) <= kRpUniMaxHalo) kd = 0;
        else kd = 3;
        if (kd == 0) halo = std::max(halo, std::abs(o));
        if (kd == 3) ++nfar;
        u.off[q] = o;
        u.kind[q] = kd;
      }
      // (n_cols < 2^28: the kernel's x offsets are 32-bit byte offsets, x16r)
      ok = ok && nfar <= kRpUniFar && A->n_cols >= 2 && A->n_cols < (int64_t(1) << 28);
      u.k = ok ? (int32_t)offs.size() : 0;
      auto kinds_are = [&](std::initializer_list<int> ks) {
        if ((size_t)u.k != ks.size()) return false;
        int q = 0;
        for (int kd : ks)
          if (u.kind[q++] != kd) return false;
        return true;
      };
      {
        // chunks of 256 pairs per workgroup: 2 (round 4: the C4 bench 1,292-1,318 -> 1,328-1,331
        // V-cycles/s against 4 on one box, same cold SpMV time; profiles/r04/uni_lab/wpe_ab.log);
        // MLAMG_RPU_CH = 1 | 2 | 4 is the A/B knob
        const char* ec = std::getenv("MLAMG_RPU_CH");
        const int chv = ec ? std::atoi(ec) : 2;
        u.ch = (chv == 1 || chv == 4) ? chv : 2;
        const char* ep = std::getenv("MLAMG_RPU_LDSPAD");  // A/B knob: caps workgroups per CU
        A->rp_lds_pad = ep ? std::max(0, std::min(std::atoi(ep), 96 << 10)) : 0;
      }
      u.layout = kinds_are({3, 0, 1, 0, 2, 0, 3}) ? 1
                 : kinds_are({0, 1, 0, 2, 0})     ? 2
                 : kinds_are({3, 1, 0, 2, 3})     ? 3
                                                  : 0;
      u.halo = ok ? halo : 0;
      if (!ok) {
        u = RpUni{};
        msk.clear();
      }
      return ok;
    };
    // alternate far offsets (a row-partitioned slab, csrc/dhier.hip's x_ext = [owned | ghosts]):
    // a ghost plane's entries reach x at an offset of their own (+n_own for the plane below,
    // +2F for the plane above when the plane below precedes it), unsorted in the row where the
    // plane below comes first. An extra far offset e stands for one of the two far offsets
    // nearest zero (s) when, in every pattern holding e, s is absent and the rows with e read
    // as s are in ascending order; the kernel then loads slot s from offset e on the pairs that
    // use e (a contiguous range, checked after the pairs are assigned below).
    std::vector<std::pair<int32_t, int32_t>> uni_alts;  // (e, s)
    if (!try_uni(pent, all_sorted, uni, hmsk) && !(uni_ev && uni_ev[0] == '0')) {
      std::vector<int32_t> far;
      for (auto& pe : pent)
        for (auto& en : pe)
          if ((en.fl & 3) && en.off != -1 && en.off != 1 &&
              ((en.off & 1) || std::abs(en.off) > kRpUniMaxHalo))
            far.push_back(en.off);
      std::sort(far.begin(), far.end());
      far.erase(std::unique(far.begin(), far.end()), far.end());
      int32_t fneg = 0, fpos = 0;
      for (int32_t o : far) {
        if (o < 0) fneg = o;  // the largest negative
        if (o > 0 && fpos == 0) fpos = o;  // the smallest positive
      }
      auto row_sorted = [](const std::vector<Ent>& pe, int bit) {
        bool first = true;
        int32_t prev = 0;
        for (auto& en : pe) {
          if (!(en.fl & bit)) continue;
          if (!first && en.off <= prev) return false;
          prev = en.off;
          first = false;
        }
        return true;
      };
      std::vector<std::vector<Ent>> pv = pent;
      bool okv = fneg != 0 && fpos != 0;
      for (int32_t e : far) {
        if (!okv || e == fneg || e == fpos) continue;
        int32_t pick = 0;
        for (int32_t s_cand : {fneg, fpos}) {
          bool good = true, used = false;
          for (auto& pe : pent) {
            bool has_e = false, has_s = false;
            for (auto& en : pe) {
              has_e = has_e || ((en.fl & 3) && en.off == e);
              has_s = has_s || ((en.fl & 3) && en.off == s_cand);
            }
            if (!has_e) continue;
            used = true;
            if (has_s) {
              good = false;
              break;
            }
            std::vector<Ent> t = pe;
            for (auto& en : t)
              if (en.off == e) en.off = s_cand;
            good = good && row_sorted(t, 1) && row_sorted(t, 2);
          }
          if (good && used) {
            okv = pick == 0;  // exactly one candidate
            pick = s_cand;
          }
        }
        okv = okv && pick != 0;
        if (!okv) break;
        for (auto& a : uni_alts) okv = okv && a.second != pick;  // one alternate per slot
        uni_alts.push_back({e, pick});
        for (auto& pe : pv)
          for (auto& en : pe)
            if (en.off == e) en.off = pick;
      }
      bool sorted_v = okv && !uni_alts.empty();
      for (auto& pe : pv) sorted_v = sorted_v && row_sorted(pe, 1) && row_sorted(pe, 2);
      if (!sorted_v || !try_uni(pv, true, uni, hmsk)) {
        uni = RpUni{};
        hmsk.clear();
        uni_alts.clear();
      }
      // the alternates' far ordinals (slot order) and their offsets; ranges follow the assign
      for (auto& a : uni_alts) {
        int t = 0;
        for (int q = 0; q < uni.k && uni.off[q] != a.second; ++q) t += uni.kind[q] == 3;
        uni.alt_off[t] = a.first;
      }
    }
    // patterns holding each alternate offset / its slot's own offset (pattern ids = pent order)
    std::vector<std::vector<bool>> alt_has_e, alt_has_s;
    for (auto& a : uni_alts) {
      std::vector<bool> he(pent.size(), false), hs(pent.size(), false);
      for (size_t k = 0; k < pent.size(); ++k)
        for (auto& en : pent[k]) {
          if (!(en.fl & 3)) continue;
          if (en.off == a.first) he[k] = true;
          if (en.off == a.second) hs[k] = true;
        }
      alt_has_e.push_back(he);
      alt_has_s.push_back(hs);
    }
    // the kernel's step: the longest pattern when it fits one step of 5..8 entries, else 8;
    // every pattern is padded with null entries to whole steps
    kstep = maxlen <= 5 ? 5 : (maxlen <= 8 ? (int)maxlen : 8);
    for (size_t k = 0; k < pats.size() && rc == MLAMG_OK; ++k) {
      for (auto& en : pent[k]) {
        hoff.push_back(en.off);
        hv0.push_back(en.v0);
        hv1.push_back(en.v1);
        hfl.push_back(en.fl);
      }
      while ((hoff.size() - hptr[k]) % kstep) {
        hoff.push_back(0);
        hv0.push_back(0.0);
        hv1.push_back(0.0);
        hfl.push_back((uint8_t)(pwide[k] ? 4 : 0));
      }
      if ((int)hoff.size() > kRpMaxEnt) {
        fail(MLAMG_EUNSUPPORTED, "row-pair patterns hold more than 2048 (padded) entries");
        break;
      }
      hptr[k + 1] = (int32_t)hoff.size();
    }
    for (size_t k = pats.size() + 1; k < 257; ++k) hptr[k] = (int32_t)hoff.size();
    // LDS windows of k_rowpair_win: the entries' offsets grouped into <= kRpWinMax
    // clusters (a gap of more than 2 NT rows starts a new one); cluster k is staged as rows
    // [R0 + s_k, R0 + s_k + L_k) of x, the clusters concatenated; an entry's window row is then
    // (r - R0) + woff, woff = base_k + off - s_k, kept in bits 8.. of its flags word
    std::vector<int32_t> hwoff(hoff.size(), 0);
    {
      const char* ev = std::getenv("MLAMG_RP_WIN");
      win.nt = kRpWinNT;
      std::vector<int32_t> offs;
      for (size_t e = 0; e < hoff.size(); ++e) offs.push_back(hoff[e]);
      std::sort(offs.begin(), offs.end());
      offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
      // opt-in (MLAMG_RP_WIN=1): on C4 this kernel measured slower than k_rowpair
      bool ok = ev && ev[0] == '1' && !offs.empty();
      std::vector<std::pair<int32_t, int32_t>> cl;  // (lo, hi) offsets
      for (int32_t o : offs) {
        if (cl.empty() || (int64_t)o - cl.back().second > 2 * win.nt)
          cl.push_back({o, o});
        else
          cl.back().second = o;
      }
      ok = ok && cl.size() <= (size_t)kRpWinMax;
      int32_t total = 0;
      for (size_t k = 0; ok && k < cl.size(); ++k) {
        const int32_t s0 = cl[k].first & ~1;                               // even start
        const int32_t len = ((2 * win.nt + cl[k].second - s0) + 1) & ~1;   // even length
        win.s[k] = s0;
        win.len[k] = len;
        win.base[k] = total;
        total += len;
      }
      // only the cluster holding offset 0 is staged (the workgroup's own rows and their
      // near neighbours); entries of the other clusters (C4: +-n^2) stay 16-byte global loads,
      // marked by flag 8 (staging them as well cost more than it saved: 3.9 rows staged per
      // row of x)
      int kc = -1;
      for (size_t k = 0; ok && k < cl.size(); ++k)
        if (cl[k].first <= 0 && 0 <= cl[k].second) kc = (int)k;
      ok = ok && kc >= 0 && win.len[kc] <= kRpWinMaxRows;
      win.n = ok ? 1 : 0;
      if (ok) {
        win.s[0] = win.s[kc];
        win.len[0] = win.len[kc];
        win.base[0] = 0;
      }
      win.rows = ok ? win.len[0] : -1;
      win.woff0 = ok ? -win.s[0] : -1;
      if (ok)
        for (size_t e = 0; e < hoff.size(); ++e) {
          if (cl[kc].first <= hoff[e] && hoff[e] <= cl[kc].second)
            hwoff[e] = hoff[e] - win.s[0];
          else
            hfl[e] |= 8;
        }
      // the kernel holds at most kRpWinG global entries per step (of kstep entries)
      for (size_t e0 = 0; ok && e0 < hoff.size(); e0 += kstep) {
        int ng = 0;
        for (size_t e = e0; e < std::min(hoff.size(), e0 + kstep); ++e) ng += (hfl[e] & 8) ? 1 : 0;
        ok = ng <= kRpWinG;
      }
      if (!ok) {
        for (auto& f : hfl) f &= ~8;
        win.n = 0;
        win.rows = -1;
      }
    }
    const size_t ne = hoff.size(), na = std::max<size_t>(ne, 1);
    // interleaved records: (offset, flags) and (row 2i value, row 2i+1 value)
    std::vector<int32_t> hof(4 * ne);
    std::vector<double> hvv(2 * ne);
    for (size_t e = 0; e < ne; ++e) {
      hof[4 * e] = hoff[e];
      hof[4 * e + 1] = (hfl[e] & 1) ? -1 : 0;
      hof[4 * e + 2] = (hfl[e] & 2) ? -1 : 0;
      hof[4 * e + 3] = hfl[e] | (win.rows >= 0 ? hwoff[e] << 8 : 0);
      hvv[2 * e] = hv0[e];
      hvv[2 * e + 1] = hv1[e];
    }
    if (rc == MLAMG_OK &&
        (hipMalloc(&poff, sizeof(int32_t) * 4 * na) != hipSuccess ||
         hipMalloc(&pval, sizeof(double) * 2 * na) != hipSuccess))
      fail(MLAMG_ENOMEM, "out of device memory");
    if (rc == MLAMG_OK &&
        (hipMemcpyAsync(pptr, hptr.data(), sizeof(int32_t) * 257, hipMemcpyHostToDevice, s) != hipSuccess ||
         (ne && (hipMemcpyAsync(poff, hof.data(), sizeof(int32_t) * 4 * ne, hipMemcpyHostToDevice, s) != hipSuccess ||
                 hipMemcpyAsync(pval, hvv.data(), sizeof(double) * 2 * ne, hipMemcpyHostToDevice, s) != hipSuccess)) ||
         hipMemcpyAsync(slot_pid, hslot.data(), sizeof(int32_t) * kDictSlots, hipMemcpyHostToDevice, s) != hipSuccess ||
         hipMemsetAsync(counts, 0, sizeof(int32_t) * 4, s) != hipSuccess))
      fail(MLAMG_EHIP, "upload");
    if (rc == MLAMG_OK && n_pairs)
      hipLaunchKernelGGL(k_rp_assign, dim3(nb), dim3(256), 0, s, A->indptr, A->indices, A->data,
                         n, A->n_cols, n_pairs, tab, slot_pid, pptr, poff, pval, pid, counts);
    if (rc == MLAMG_OK &&
        (hipGetLastError() != hipSuccess ||
         hipMemcpyAsync(hc, counts, sizeof(hc), hipMemcpyDeviceToHost, s) != hipSuccess ||
         hipStreamSynchronize(s) != hipSuccess))
      fail(MLAMG_EHIP, "assign");
    if (rc == MLAMG_OK && hc[0] != 0)
      fail(MLAMG_EUNSUPPORTED, "row-pair pattern hash collision");
    // the alternates' pair ranges: the pairs whose pattern holds e must form one run in which no
    // pair's pattern holds the slot's own offset (the kernel switches the slot's offset by pair
    // range); otherwise no uniform form (the general row-pair kernel reads actual offsets)
    if (rc == MLAMG_OK && !uni_alts.empty()) {
      std::vector<uint8_t> hp((size_t)n_pairs);
      bool okr = hipMemcpy(hp.data(), pid, (size_t)n_pairs, hipMemcpyDeviceToHost) == hipSuccess;
      for (size_t a = 0; okr && a < uni_alts.size(); ++a) {
        int64_t lo = -1, hi = -1;
        for (int64_t i = 0; i < n_pairs; ++i)
          if (alt_has_e[a][hp[i]]) {
            if (lo < 0) lo = i;
            hi = i + 1;
          }
        okr = lo >= 0;
        for (int64_t i = lo; okr && i < hi; ++i) okr = !alt_has_s[a][hp[i]];
        int t = 0;
        for (int q = 0; q < uni.k && uni.off[q] != uni_alts[a].second; ++q) t += uni.kind[q] == 3;
        uni.alt_lo[t] = (int32_t)lo;
        uni.alt_hi[t] = (int32_t)hi;
      }
      if (!okr) {
        uni = RpUni{};
        hmsk.clear();
      } else {
        // the compile-time layouts without alternates never compare pair ranges
        uni.layout = uni.layout == 1 ? 4 : 0;
      }
    }
  }
  for (void* p : {(void*)tab, (void*)rep, (void*)counts, (void*)slot_pid})
    if (p) (void)hipFree(p);
  if (rc != MLAMG_OK) {
    for (void* p : {(void*)pid, (void*)pptr, (void*)poff, (void*)pval})
      if (p) (void)hipFree(p);
    return rc;
  }
  // k_rowpair_win's slot order: within each workgroup's 256 pairs, the pairs sorted (stably) by
  // pattern, each slot a uint16 (pattern | local pair << 8), so a wave's lanes share a pattern
  // and read its records with scalar loads
  uint16_t* pslot = nullptr;
  if (win.rows >= 0 && n_pairs > 0) {
    std::vector<uint8_t> hp((size_t)n_pairs);
    std::vector<uint16_t> hs((size_t)n_pairs);
    bool okc = hipMemcpy(hp.data(), pid, (size_t)n_pairs, hipMemcpyDeviceToHost) == hipSuccess;
    for (int64_t c0 = 0; okc && c0 < n_pairs; c0 += kRpWinNT) {
      const int64_t c1 = std::min<int64_t>(n_pairs, c0 + kRpWinNT);
      int cnt[257] = {0};
      for (int64_t i = c0; i < c1; ++i) ++cnt[hp[i] + 1];
      for (int k = 0; k < 256; ++k) cnt[k + 1] += cnt[k];
      for (int64_t i = c0; i < c1; ++i)
        hs[c0 + cnt[hp[i]]++] = (uint16_t)(hp[i] | ((i - c0) << 8));
    }
    okc = okc && hipMalloc(&pslot, sizeof(uint16_t) * (size_t)n_pairs) == hipSuccess &&
          hipMemcpy(pslot, hs.data(), sizeof(uint16_t) * (size_t)n_pairs,
                    hipMemcpyHostToDevice) == hipSuccess;
    if (!okc) {
      if (pslot) (void)hipFree(pslot);
      pslot = nullptr;
      win = RpWin{};
    }
  }
  uint16_t* pmsk = nullptr;
  if (uni.k > 0) {
    hmsk.resize(256, 0);
    if (hipMalloc(&pmsk, sizeof(uint16_t) * 256) != hipSuccess ||
        hipMemcpy(pmsk, hmsk.data(), sizeof(uint16_t) * 256, hipMemcpyHostToDevice) != hipSuccess) {
      if (pmsk) (void)hipFree(pmsk);
      pmsk = nullptr;
      uni = RpUni{};
    }
  }
  drop_rowpat(A);
  A->rp_uni = uni;
  // plane-marching form (k_rowpat_march): the 3-D 7-point layout with its far offsets one even
  // plane of rows F apart. Opt-in (MLAMG_RPM=1: slower than k_rowpat_uni so far, DESIGN.md
  // §13); MLAMG_RPM_CH (1 | 2 | 4) and MLAMG_RPM_SEG
  // (planes per segment; 0 = enough workgroups for two (CH 4) / four (CH 2) per CU) are A/B knobs
  if (uni.k == 7 && uni.layout == 1 && A->n_rows == A->n_cols && uni.off[6] > 0 &&
      uni.alt_hi[0] == uni.alt_lo[0] && uni.alt_hi[1] == uni.alt_lo[1] &&
      uni.off[0] == -uni.off[6] && (uni.off[6] & 1) == 0 && uni.off[6] >= 2048 &&
      A->n_rows >= 3 * (int64_t)uni.off[6]) {
    const char* e0 = std::getenv("MLAMG_RPM");
    const char* e1 = std::getenv("MLAMG_RPM_CH");
    const char* e2 = std::getenv("MLAMG_RPM_SEG");
    if (e0 && std::atoi(e0) == 1) {
      const int64_t F = uni.off[6];
      const int ch = e1 && (std::atoi(e1) == 1 || std::atoi(e1) == 2) ? std::atoi(e1) : 4;
      const int64_t T = 2 * ch * kThreads;
      const int64_t nt = (F + T - 1) / T, n_planes = (A->n_rows + F - 1) / F;
      const int64_t target = 256 * (ch == 4 ? 2 : ch == 2 ? 4 : 6);
      int64_t seg = e2 ? std::atoi(e2) : 0;
      if (seg <= 0) seg = std::max<int64_t>(2, (n_planes * nt + target - 1) / target);
      const char* e3 = std::getenv("MLAMG_RPM_PF");  // planes prefetched ahead (1 | 2)
      A->rp_mF = F;
      A->rp_mch = ch;
      A->rp_mpf = (e3 && std::atoi(e3) == 2 && ch <= 2) ? 2 : 1;
      A->rp_mseg = (int32_t)std::min<int64_t>(seg, n_planes);
    }
  }
  A->rp_msk = pmsk;
  A->rp_win = win;
  A->rp_slot = pslot;
  A->rp_pid = pid;
  A->rp_ptr = pptr;
  A->rp_off = poff;
  A->rp_val = pval;
  A->rp_n_pat = n_pat;
  A->rp_n_ent = (int32_t)hoff.size();
  A->rp_k = kstep;
  A->rp_rep = std::move(reps);
  return MLAMG_OK;
}

// per-pattern (dinv[2i], dinv[2i+1]) must equal the representative pair's, for every pair
__global__ void k_rp_dinv_check(const uint8_t* __restrict__ pid, const double* __restrict__ dinv,
                                const double* __restrict__ tab, int64_t n, int32_t* bad) {
  const int64_t pr = blockIdx.x * 256ll + threadIdx.x;
  if (2 * pr >= n) return;
  const int p = pid[pr];
  bool ok = __double_as_longlong(dinv[2 * pr]) == __double_as_longlong(tab[2 * p]);
  if (2 * pr + 1 < n)
    ok = ok && __double_as_longlong(dinv[2 * pr + 1]) == __double_as_longlong(tab[2 * p + 1]);
  if (!ok) atomicAdd(bad, 1);
}

void drop_formats(mlamg_csr* A, bool free_arrays) {
  drop_vector(A, free_arrays);
  drop_long(A, free_arrays);
  drop_rowpat(A, free_arrays);
  drop_sorted(A, free_arrays);
  drop_sell(A, free_arrays);
  A->n_part = A->n_blocks;
}

// SELL-64 in natural row order if its padding costs <= 15% extra entries, else SELL-64-sigma
// (rows sorted by length inside windows of 512) if that does, else CSR-stream
static int build_auto_exact(mlamg_csr* A, hipStream_t s) {
  for (int sigma : {1, 512}) {
    MLAMG_TRY(build_sell(A, s, sigma));
    if (A->nnz > 0 && (double)A->sell_elems <= 1.15 * (double)A->nnz) return MLAMG_OK;
  }
  drop_sell(A);
  return MLAMG_OK;
}

}  // namespace mlamg

using namespace mlamg;

extern "C" {

int mlamg_csr_set_format(mlamg_csr* A, int fmt, int vec_width, void* stream) {
  MLAMG_REQUIRE(A, "NULL argument");
  hipStream_t s = S(stream);
  bump_format_epoch();
  int vw = vec_width;
  if (fmt == MLAMG_FMT_SORTED) {
    // vec_width 2: fp64 values replaced by two-byte value codes, EUNSUPPORTED where they do
    // not apply
    MLAMG_REQUIRE(vec_width == 0 || vec_width == 1 || vec_width == 2,
                  "sorted: vec_width must be 0/1 (values or dictionary) or 2 (value codes)");
  } else if (fmt == MLAMG_FMT_VECTOR) {
    if (vw == 0) {  // auto: a wave per 128 entries of the mean row, 64..512 lanes
      vw = 64;
      while (vw < 512 && 2.0 * vw <= A->avg_row_len) vw *= 2;
    }
    MLAMG_REQUIRE(vw == 64 || vw == 128 || vw == 256 || vw == 512,
                  "vec_width must be 0 (auto), 64, 128, 256 or 512");
    if (A->n_rows > kWideMaxRows) {
      set_error("the VECTOR format needs <= 2^20 rows");
      return MLAMG_EUNSUPPORTED;
    }
  }
  // The current format is set aside (`old` owns its arrays) and the new one is built on the
  // handle as plain CSR-stream: a refused or failed conversion puts `old` back, so the handle is
  // then exactly as it was, whatever format it was in.
  mlamg_csr old = *A;
  drop_formats(A, /*free_arrays=*/false);
  int rc = MLAMG_OK;
  switch (fmt) {
    case MLAMG_FMT_CSR_STREAM: break;
    case MLAMG_FMT_SELL:  // vec_width doubles as sigma
      rc = build_sell(A, s, vec_width > 1 ? vec_width : 1);
      break;
    case MLAMG_FMT_SELL_DICT: rc = build_sell_dict(A, s, vec_width > 1 ? vec_width : 1); break;
    case MLAMG_FMT_SORTED: rc = build_sorted(A, s, vec_width); break;
    case MLAMG_FMT_LONG: rc = build_long(A, s); break;
    case MLAMG_FMT_VECTOR:
      A->vec_width = vw;
      rc = build_vec16(A, s);
      break;
    case MLAMG_FMT_AUTO_EXACT: rc = build_auto_exact(A, s); break;
    case MLAMG_FMT_ROWPAT: rc = build_rowpat(A, s); break;
    default: set_error("mlamg_csr_set_format: unknown format"); rc = MLAMG_EINVAL;
  }
  if (rc != MLAMG_OK) {
    drop_formats(A);
    *A = std::move(old);
    return rc;
  }
  drop_formats(&old);
  A->n_part = norm_partials(A);
  return MLAMG_OK;
}

int mlamg_csr_format_bytes(const mlamg_csr* A, double* bytes) {
  MLAMG_REQUIRE(A && bytes, "NULL argument");
  const double n = (double)A->n_rows, m = (double)A->n_cols;
  double b = 8.0 * m + 8.0 * n;  // x read once, y written once
  const int fmt = active_format(A);
  if (fmt == MLAMG_FMT_VECTOR) {
    b += (A->vec_idx16 ? 10.0 : 12.0) * A->nnz + 4.0 * (n + 1);
  } else if (fmt == MLAMG_FMT_LONG) {
    b += 12.0 * A->nnz + 4.0 * (n + 1) + 4.0 * (A->lg_nt + 1);
  } else if (rowpat_uniform(A)) {
    b += 1.0 * ((A->n_rows + 1) / 2) + 2.0 * 256;  // pair ids + the mask table
  } else if (fmt == MLAMG_FMT_ROWPAT) {
    b += 1.0 * ((A->n_rows + 1) / 2) + 4.0 * 257 + 32.0 * A->rp_n_ent;  // pair ids + tables
  } else if (fmt == MLAMG_FMT_SORTED) {
    b += (A->srt_vi ? 5.0 : A->srt_vc ? 6.0 : 12.0) * (double)kSrtNnz * A->srt_nb +
         4.0 * (n + 1) + 32.0 * A->srt_nb;  // the padded fixed-stride stream
    if (A->srt_vc) b += 8.0 * (double)A->srt_vtab_n + 8.0 * A->srt_nb;  // dictionaries
  } else if (fmt == MLAMG_FMT_SELL_DICT) {
    int64_t n_codes = 0;
    MLAMG_HIP(hipMemcpy(&n_codes, A->dict_ptr + A->n_slices, sizeof(int64_t), hipMemcpyDeviceToHost));
    b += 2.0 * n_codes + 8.0 * (A->n_slices + 1) + (A->sell_perm ? 4.0 * n : 0.0) +
         256.0 * 12.0;
  } else if (fmt == MLAMG_FMT_SELL) {
    b += 12.0 * A->sell_elems + 8.0 * (A->n_slices + 1) + (A->sell_perm ? 4.0 * n : 0.0);
  } else {
    b += 12.0 * A->nnz + 4.0 * (n + 1);
  }
  *bytes = b;
  return MLAMG_OK;
}

int mlamg_csr_attach_dinv(mlamg_csr* A, const double* dinv_w, void* stream) {
  MLAMG_REQUIRE(A, "NULL argument");
  hipStream_t s = S(stream);
  bump_format_epoch();
  if (A->rp_dinv) (void)hipFree(A->rp_dinv);
  A->rp_dinv = nullptr;
  A->rp_dinv_att = nullptr;
  if (!dinv_w) return MLAMG_OK;  // detach
  if (!A->rp_pid) {
    set_error("attach_dinv: the operator is not in rowpat format");
    return MLAMG_EUNSUPPORTED;
  }
  const int np = A->rp_n_pat;
  const int64_t n = A->n_rows;
  std::vector<double> tab(2 * std::max(np, 1), 0.0);
  for (int p = 0; p < np; ++p) {
    const int64_t r0 = 2 * (int64_t)A->rp_rep[p];
    MLAMG_HIP(hipMemcpy(&tab[2 * p], dinv_w + r0, sizeof(double) * (r0 + 1 < n ? 2 : 1),
                        hipMemcpyDeviceToHost));
  }
  double* d = nullptr;
  int32_t* bad = nullptr;
  MLAMG_HIP(hipMalloc(&d, sizeof(double) * tab.size()));
  if (hipMalloc(&bad, sizeof(int32_t)) != hipSuccess) {
    (void)hipFree(d);
    set_error("attach_dinv: out of device memory");
    return MLAMG_ENOMEM;
  }
  int32_t hb = 0;
  hipError_t e = hipMemcpyAsync(d, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, sizeof(int32_t), s);
  const int64_t n_pairs = (n + 1) / 2;
  if (e == hipSuccess && n_pairs) {
    hipLaunchKernelGGL(k_rp_dinv_check, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s,
                       A->rp_pid, dinv_w, d, n, bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&hb, bad, sizeof(int32_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(bad);
  if (e != hipSuccess || hb != 0) {
    (void)hipFree(d);
    if (e != hipSuccess) {
      set_error(std::string("attach_dinv: ") + hipGetErrorString(e));
      return MLAMG_EHIP;
    }
    set_error("attach_dinv: dinv is not constant over the operator's row-pair patterns");
    return MLAMG_EUNSUPPORTED;
  }
  A->rp_dinv = d;
  A->rp_dinv_att = dinv_w;
  return MLAMG_OK;
}

int mlamg_csr_get_format(const mlamg_csr* A, int* fmt, int* vec_width, int64_t* stored) {
  MLAMG_REQUIRE(A, "NULL argument");
  const int f = active_format(A);
  if (fmt) *fmt = f;
  // SORTED reports 1 in vec_width when its values are dictionary-coded, 2 for value codes
  if (vec_width)
    *vec_width = f == MLAMG_FMT_VECTOR   ? A->vec_width
                 : f == MLAMG_FMT_ROWPAT ? A->rp_n_pat
                 : f == MLAMG_FMT_SORTED ? (A->srt_vi ? 1 : A->srt_vc ? 2 : 0)
                                         : A->sell_sigma;
  if (stored) *stored = A->sell_ptr ? A->sell_elems : A->nnz;
  return MLAMG_OK;
}

}  // extern "C"
