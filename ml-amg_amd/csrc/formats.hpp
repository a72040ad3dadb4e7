// The seam between the SpMV kernels (spmv.hip) and the storage-format construction
// (formats.hip): which format a handle is in, and how its format arrays are released.
#pragma once

#include "common.hpp"

namespace mlamg {

// The active storage format (MLAMG_FMT_*). A handle holds at most one format's arrays besides
// its CSR arrays; this is the one place their precedence is written.
inline int active_format(const mlamg_csr* A) {
  return A->vec_width   ? MLAMG_FMT_VECTOR
         : A->lg_tile   ? MLAMG_FMT_LONG
         : A->rp_pid    ? MLAMG_FMT_ROWPAT
         : A->srt_pk    ? MLAMG_FMT_SORTED
         : A->dict_code ? MLAMG_FMT_SELL_DICT
         : A->sell_ptr  ? MLAMG_FMT_SELL
                        : MLAMG_FMT_CSR_STREAM;
}

// ROWPAT in its uniform-stencil form (k_rowpat_uni). build_rowpat clears rp_uni when the mask
// table cannot be allocated and drop_rowpat resets both, so rp_uni.k > 0 implies rp_msk.
inline bool rowpat_uniform(const mlamg_csr* A) {
  return A->rp_pid && A->rp_uni.k > 0 && A->rp_msk;
}

// Back to plain CSR-stream: every format's arrays freed and forgotten (attached Jacobi weights
// included), n_part restored. free_arrays = false only forgets them: for a handle whose arrays
// another copy of the struct now owns (mlamg_csr_set_format sets the current format aside so).
void drop_formats(mlamg_csr* A, bool free_arrays = true);

// Norm partials a NORM launch writes with the active format (spmv.hip: mirrors the grid sizes).
int32_t norm_partials(const mlamg_csr* A);

}  // namespace mlamg
