// shard_exec.cpp — what qsim_cluster (cluster.cpp) and qsim_rank_comm (rank_comm.cpp) execute a plan with: the error channel,
// the refusals, a local step onto a state or into a circuit, and one shard's RCCL leg of an exchange (shard_plan.h).
#include <cstdarg>
#include <cstdio>

#include "qsim_internal.h"
#include "shard_exec.h"

namespace shard {

thread_local std::string g_derr;
int cfail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_derr = buf;
    return code;
}

int check_shards(int num_q, int num_shards, int *p_out) {
    int p = 0;
    while ((1 << p) < num_shards) p++;
    if (num_shards < 1 || (1 << p) != num_shards) return cfail(QSIM_ERR_ARG, "shard count %d is not a power of two", num_shards);
    if (num_q - p < 2 && p > 0) return cfail(QSIM_ERR_ARG, "%d qubits cannot be split over %d shards", num_q, num_shards);
    if (p > kMaxRoleBits) return cfail(QSIM_ERR_ARG, "%d shards: at most %d are supported (an exchange has one mask bit per block of a group)", num_shards, 1 << kMaxRoleBits);
    *p_out = p;
    return QSIM_OK;
}

int check_shardable(const qsim_circuit *circ, int n_expected, const char *where) {
    if (n_expected >= 0 && circ->num_q != n_expected) return cfail(QSIM_ERR_ARG, "circuit has %d qubits, cluster has %d", circ->num_q, n_expected);
    for (long i = 0; i < circ->count; i++)
        if (circ->gates[i].kind == QSIM_GATE_U2) return cfail(QSIM_ERR_ARG, "generic 2-qubit gates are not supported on %s", where);
    return QSIM_OK;
}

namespace {
struct StateSink { // the engine's gate queue
    qsim_state *s;
    int cx(int a, int b) { return qsim_apply_cx(s, a, b); }
    int u1(const cd *m, int a) { return qsim_apply_1q(s, as_doubles(m), a); }
    int scale(cd z) { return qsim_scale(s, z.real(), z.imag()); }
};
struct CircuitSink { // a circuit has no scalar multiply
    qsim_circuit *c;
    int cx(int a, int b) { return qsim_circuit_append_cx(c, a, b); }
    int u1(const cd *m, int a) { return qsim_circuit_append_1q(c, as_doubles(m), a); }
    int scale(cd z) { return scale_as_gate(*this, z); }
};
} // namespace

int apply_ops(qsim_state *s, const std::vector<LocalOp> &ops) {
    const int rc = replay(ops, StateSink{s});
    return rc ? cfail(rc, "%s", qsim_last_error()) : QSIM_OK;
}

int step_circuit(const std::vector<LocalOp> &ops, int m, qsim_circuit **out) {
    qsim_circuit *c = nullptr;
    int rc = qsim_circuit_create(m, &c);
    if (rc == QSIM_OK) rc = replay(ops, CircuitSink{c});
    if (rc) { qsim_circuit_free(c); return rc; }
    *out = c;
    return QSIM_OK;
}

int settle(qsim_state *s, const Roles &r) {
    return r.empty_after ? qsim_reset_shard(s, 0) : qsim_set_support(s, r.new_support);
}

int pack_or_flush(qsim_state *s, const Step &st, const Roles &ro, const int *to, uint64_t konst, void *out, PackCounts &counts) {
    int fused = 0;
    const int rc = ro.empty_before ? qsim_flush(s) : qsim_flush_pack(s, st.Lsel.data(), (int)st.J.size(), to, konst, out, st.mixed_local, ro.unread, nullptr, &fused);
    if (rc) return cfail(rc, "%s", qsim_last_error());
    if (!ro.empty_before) (fused ? counts.fused : counts.separate)++;
    return QSIM_OK;
}

ncclResult_t post_transfers(qsim_state *s, const Roles &ro, int k, const void *scratch, void *state, ncclComm_t comm) {
    const size_t blk = blk_bytes(qsim_num_qubits(s), k);
    hipStream_t stream = (hipStream_t)qsim_stream(s);
    ncclResult_t nr = ncclSuccess;
    for (int b = 0; b < (1 << k) && nr == ncclSuccess; b++) {
        if (ro.send >> b & 1u) nr = ncclSend((const char *)scratch + (size_t)b * blk, blk / 8, ncclDouble, ro.members[b], comm, stream);
        if (nr == ncclSuccess && (ro.recv >> b & 1u)) nr = ncclRecv((char *)state + (size_t)b * blk, blk / 8, ncclDouble, ro.members[b], comm, stream);
    }
    return nr;
}

int keep_own_and_settle(qsim_state *s, const Roles &ro, int k, const void *scratch, void *state) {
    const size_t blk = blk_bytes(qsim_num_qubits(s), k), at = (size_t)ro.mine * blk;
    if (ro.keep_own && hipMemcpyAsync((char *)state + at, (const char *)scratch + at, blk, hipMemcpyDeviceToDevice, (hipStream_t)qsim_stream(s)) != hipSuccess)
        return cfail(QSIM_ERR_DEVICE, "exchange copy failed");
    const int rc = settle(s, ro);
    return rc ? cfail(rc, "%s", qsim_last_error()) : QSIM_OK;
}

} // namespace shard
