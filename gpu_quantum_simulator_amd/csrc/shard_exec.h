// shard_exec.h — one shard's RCCL leg of an exchange, shared by qsim_cluster (cluster.cpp, for each shard) and qsim_rank_comm
// (rank_comm.cpp, for its rank) and defined in shard_exec.cpp.  Apart from shard_plan.h because it needs <rccl/rccl.h>.
#ifndef QSIM_SHARD_EXEC_H
#define QSIM_SHARD_EXEC_H

#include <rccl/rccl.h>

#include "shard_plan.h"

namespace shard __attribute__((visibility("hidden"))) {

// One shard's leg of an exchange, in three pieces; the callers keep what differs between them (which group of sends and receives
// is open, timing, refusals).
struct PackCounts { uint64_t fused = 0, separate = 0; };
// 1. A shard that holds nothing drops its queue; any other launches it with the last tile pass writing the packed layout where
//    it can (qsim_flush_pack; to / konst / out as there), and counts which it was.
int pack_or_flush(qsim_state *s, const Step &st, const Roles &ro, const int *to, uint64_t konst, void *out, PackCounts &counts);
// 2. Inside the caller's open group, on the shard's stream: the sends of its packed blocks (scratch) and the receives into its
//    state buffer.
ncclResult_t post_transfers(qsim_state *s, const Roles &ro, int k, const void *scratch, void *state, ncclComm_t comm);
// 3. The block the shard keeps, then settle().
int keep_own_and_settle(qsim_state *s, const Roles &ro, int k, const void *scratch, void *state);

} // namespace shard

#endif
