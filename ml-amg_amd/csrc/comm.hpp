// The seam between the multi-GPU transport (comm.hip) and the partitioned V-cycle executor
// (dhier.hip): the transport calls, and the few facts the executor reads of a communicator and
// of a halo. The executor sees neither RCCL nor the loopback transport's types.
#pragma once
#include "common.hpp"

namespace mlamg {

// ---------------------------------------------------------------- communicator
int comm_rank(const mlamg_comm* c);
int comm_size(const mlamg_comm* c);
// the in-process test transport: host threads meeting in a mailbox, which no graph can capture
bool comm_is_loopback(const mlamg_comm* c);

// Grouped point-to-point messages of doubles and a sum all-reduce, on stream s: RCCL's
// ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd / ncclAllReduce semantics on every
// transport (message order per peer pair, nothing completes before the group ends).
int xgroup_begin(mlamg_comm* c);
int xsend(mlamg_comm* c, const double* buf, size_t n, int peer, hipStream_t s);
int xrecv(mlamg_comm* c, double* buf, size_t n, int peer, hipStream_t s);
int xgroup_end(mlamg_comm* c, hipStream_t s);
int xallreduce_sum(mlamg_comm* c, double* buf, size_t n, hipStream_t s);

// ---------------------------------------------------------------- halo
// x_ext = [owned rows | ghost rows]: the owned entries the neighbours need are packed into the
// halo's send buffer, and the grouped exchange fills the ghost rows.
int64_t halo_owned(const mlamg_halo* h);
int64_t halo_ghosts(const mlamg_halo* h);
bool halo_has_neighbours(const mlamg_halo* h);
int halo_pack(mlamg_halo* h, const double* x_ext, hipStream_t s);
int halo_post(mlamg_halo* h, double* x_ext, hipStream_t s);  // needs the pack, on any stream
int halo_exchange_impl(mlamg_halo* h, double* x_ext, hipStream_t s);  // pack, then post

}  // namespace mlamg
