// rank_comm.cpp — one process per GPU: this rank's end of the exchanges, on RCCL, and the qsim_shard_plan functions that work on
// a shard's qsim_state (shard_plan.h says who owns what).
// The launcher's own channel (torch.distributed, MPI, a file) only carries the 128-byte RCCL id from rank 0 to the
// others; every byte of state travels through ncclSend / ncclRecv issued here, on the shard's own stream, behind the
// pack kernel and in front of the next pass — no host synchronisation inside an exchange.
#include <cstring>

#include "qsim_internal.h"
#include "shard_exec.h"

using namespace shard;

struct qsim_rank_comm {
    ncclComm_t comm = nullptr;
    qsim_state *shard = nullptr;
    int world = 0, rank = 0, device = 0;
    void *scratch = nullptr;
    bool owns_scratch = false;
    uint64_t exchanges = 0;
    PackCounts packs;
    double bytes_sent = 0, ms = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timing; // start/stop of exchanges not yet resolved
};

static_assert(sizeof(ncclUniqueId) == QSIM_RCCL_ID_BYTES, "QSIM_RCCL_ID_BYTES must equal sizeof(ncclUniqueId)");

extern "C" int qsim_rccl_unique_id(void *id) {
    if (!id) return cfail(QSIM_ERR_ARG, "NULL argument");
    ncclUniqueId uid;
    const ncclResult_t nr = ncclGetUniqueId(&uid);
    if (nr != ncclSuccess) return cfail(QSIM_ERR_DEVICE, "ncclGetUniqueId failed: %s", ncclGetErrorString(nr));
    memcpy(id, &uid, sizeof uid);
    return QSIM_OK;
}

extern "C" void qsim_rank_comm_destroy(qsim_rank_comm *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->shard) (void)qsim_sync(c->shard);
    for (auto &pr : c->timing) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->owns_scratch && c->scratch) (void)hipFree(c->scratch);
    delete c;
}

extern "C" int qsim_rank_comm_create(qsim_rank_comm **out, qsim_state *shard, int device, int world, int rank, const void *id, void *scratch) {
    if (!out || !shard || !id) return cfail(QSIM_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (world < 1 || (world & (world - 1)) || rank < 0 || rank >= world) return cfail(QSIM_ERR_ARG, "bad world size / rank (%d, %d)", world, rank);
    if (qsim_precision_bits(shard) != 64) return cfail(QSIM_ERR_ARG, "sharded states are fp64");
    qsim_rank_comm *c = new qsim_rank_comm();
    c->shard = shard; c->world = world; c->rank = rank; c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return cfail(QSIM_ERR_DEVICE, "hipSetDevice(%d) failed", device); }
    if (scratch) c->scratch = scratch;
    else {
        if (hipMalloc(&c->scratch, (size_t)16 << qsim_num_qubits(shard)) != hipSuccess) { delete c; return cfail(QSIM_ERR_ALLOC, "Malloc error"); }
        c->owns_scratch = true;
    }
    (void)qsim_set_option(shard, QSIM_OPT_DEFER_FLIPS, 0); // a shard's last pass may have to do an exchange's re-layout
    (void)qsim_set_spare_buffer(shard, c->scratch); // idle between exchanges: the second buffer of the shard's out-of-place passes
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    const ncclResult_t nr = ncclCommInitRank(&c->comm, world, uid, rank);
    if (nr != ncclSuccess) {
        c->comm = nullptr;
        qsim_rank_comm_destroy(c);
        return cfail(QSIM_ERR_DEVICE, "ncclCommInitRank failed: %s", ncclGetErrorString(nr));
    }
    *out = c;
    return QSIM_OK;
}

// Swaps k rank-id bits (st.J, ascending) with k local bits (st.Lsel, ascending) of this rank's shard; st.mixed_* say where the
// register can be non-zero (all ones: anywhere), see roles_of.
static int rank_exchange(qsim_rank_comm *c, const Step &st) {
    const int k = (int)st.J.size();
    const int m = qsim_num_qubits(c->shard);
    if (k < 1 || k > m || k > kMaxRoleBits || (1 << k) > c->world) return cfail(QSIM_ERR_ARG, "exchange of %d qubits unsupported here (at most %d: groups of %d ranks)", k, kMaxRoleBits, 1 << kMaxRoleBits);
    for (int j : st.J)
        if (j < 0 || (1 << j) >= c->world) return cfail(QSIM_ERR_ARG, "rank bit %d outside the world", j);
    const Roles ro = roles_of(c->rank, m, st);
    // The plan says this rank holds nothing here; that is only true on a run from |0...0> (qsim_reset_shard, then the plan's
    // steps in order).  A shard that was written since would silently lose its amplitudes: refuse.
    if (ro.empty_before && !qsim_holds_nothing(c->shard))
        return cfail(QSIM_ERR_ARG, "the plan's exchange assumes a run from |0...0> (this rank should hold nothing here and does): reset the shards, then run the plan's steps in order");
    if (hipSetDevice(c->device) != hipSuccess) return cfail(QSIM_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t stream = (hipStream_t)qsim_stream(c->shard);
    // exchanges are timed (HIP events on the shard's stream) only while the shard is in profile mode, and never more
    // than a bounded number of them stay unresolved: a long-running program that never asks for the statistics must
    // not collect events
    const bool timed = qsim_get_option(c->shard, QSIM_OPT_PROFILE) != 0 && c->timing.size() < 4096;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timed && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) return cfail(QSIM_ERR_DEVICE, "event creation failed");
    // Everything queued so far belongs in front of the exchange, and the last tile pass of it writes the state straight into
    // the packed layout where it can (qsim_flush_pack): the exchange then costs no sweep of its own.  (The timing below
    // therefore starts behind that pass: what it measures is the transfer, plus the pack kernel when one had to run.)
    if (int rc = pack_or_flush(c->shard, st, ro, nullptr, 0, c->scratch, c->packs)) return rc;
    if (timed) (void)hipEventRecord(e0, stream);
    void *state = qsim_state_buffer(c->shard);
    if (ro.send | ro.recv) {
        ncclResult_t nr = ncclGroupStart();
        if (nr == ncclSuccess) nr = post_transfers(c->shard, ro, k, c->scratch, state, c->comm);
        const ncclResult_t ne = ncclGroupEnd();
        if (nr == ncclSuccess) nr = ne;
        if (nr != ncclSuccess) return cfail(QSIM_ERR_DEVICE, "RCCL exchange failed: %s", ncclGetErrorString(nr));
    }
    if (int rc = keep_own_and_settle(c->shard, ro, k, c->scratch, state)) return rc;
    if (timed) {
        (void)hipEventRecord(e1, stream);
        c->timing.emplace_back(e0, e1);
    }
    c->exchanges++;
    c->bytes_sent += (double)blk_bytes(m, k) * __builtin_popcount(ro.send);
    return QSIM_OK;
}

extern "C" int qsim_rank_comm_exchange(qsim_rank_comm *c, const int *shard_bits, const int *local_bits, int k) {
    if (!c || !shard_bits || !local_bits) return cfail(QSIM_ERR_ARG, "NULL argument");
    if (k < 1 || k > kMaxRoleBits) return cfail(QSIM_ERR_ARG, "exchange of %d qubits unsupported here (at most %d)", k, kMaxRoleBits);
    Step st;
    st.exchange = true;
    st.J.assign(shard_bits, shard_bits + k);
    st.Lsel.assign(local_bits, local_bits + k);
    st.mixed_local = st.mixed_rank = ~0ULL; // nothing is known about the contents: every block travels
    return rank_exchange(c, st);
}

// The exchange of one step of a plan, with what the plan knows about the state at that point: a run starts from |0...0>,
// so early exchanges involve shards that hold nothing and blocks that are zero throughout (Step::mixed_*); those neither
// travel nor get written, and the shard goes on visiting only the part of itself that can be non-zero.
extern "C" int qsim_rank_comm_exchange_step(qsim_rank_comm *c, const qsim_shard_plan *p, int step) {
    if (!c || !p || step < 0 || step >= (int)p->plan.steps.size()) return cfail(QSIM_ERR_ARG, "bad argument");
    const Step &st = p->plan.steps[(size_t)step];
    if (!st.exchange) return cfail(QSIM_ERR_ARG, "step %d is not an exchange", step);
    if (p->P != c->world) return cfail(QSIM_ERR_ARG, "plan for %d shards, communicator of %d ranks", p->P, c->world);
    return rank_exchange(c, st);
}

// Exchanges so far, bytes this rank sent, and the seconds its stream spent in them (pack + send/recv, HIP events on the
// shard's stream; waits for the stream).  reset != 0 clears the counters afterwards.
extern "C" int qsim_rank_comm_stats(qsim_rank_comm *c, uint64_t *exchanges, double *bytes_sent, double *seconds, int reset) {
    if (!c) return cfail(QSIM_ERR_ARG, "NULL argument");
    if (!c->timing.empty()) {
        const int rc = qsim_sync(c->shard);
        if (rc) return cfail(rc, "%s", qsim_last_error());
        for (auto &pr : c->timing) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) c->ms += ms;
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
        c->timing.clear();
    }
    if (exchanges) *exchanges = c->exchanges;
    if (bytes_sent) *bytes_sent = c->bytes_sent;
    if (seconds) *seconds = c->ms * 1e-3;
    if (reset) { c->exchanges = 0; c->bytes_sent = 0; c->ms = 0; }
    return QSIM_OK;
}

extern "C" int qsim_rank_comm_pack_counts(const qsim_rank_comm *c, uint64_t *fused, uint64_t *separate) {
    if (!c) return QSIM_ERR_ARG;
    if (fused) *fused = c->packs.fused;
    if (separate) *separate = c->packs.separate;
    return QSIM_OK;
}

// Diagnostic: the first `count` doubles of the shard travel through ncclSend -> ncclRecv to this same rank (one group, on
// the shard's stream) into the scratch buffer and are compared on the host.  It is the only way to drive the RCCL call
// path of qsim_rank_comm_exchange where a single GPU is present (a 1-rank communicator has nobody to exchange with).
extern "C" int qsim_rank_comm_loopback(qsim_rank_comm *c, uint64_t count) {
    if (!c) return cfail(QSIM_ERR_ARG, "NULL argument");
    const uint64_t cap = (uint64_t)2 << qsim_num_qubits(c->shard);
    if (count < 1 || count > cap) return cfail(QSIM_ERR_ARG, "loopback count outside the shard");
    if (hipSetDevice(c->device) != hipSuccess) return cfail(QSIM_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t stream = (hipStream_t)qsim_stream(c->shard);
    const void *state = qsim_device_ptr(c->shard);
    if (!state) return cfail(QSIM_ERR_DEVICE, "%s", qsim_last_error());
    ncclResult_t nr = ncclGroupStart();
    if (nr == ncclSuccess) nr = ncclSend(state, count, ncclDouble, c->rank, c->comm, stream);
    if (nr == ncclSuccess) nr = ncclRecv(c->scratch, count, ncclDouble, c->rank, c->comm, stream);
    const ncclResult_t ne = ncclGroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return cfail(QSIM_ERR_DEVICE, "RCCL loopback failed: %s", ncclGetErrorString(nr));
    if (hipStreamSynchronize(stream) != hipSuccess) return cfail(QSIM_ERR_DEVICE, "stream sync failed");
    std::vector<double> a(count), b(count);
    if (hipMemcpy(a.data(), state, count * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(b.data(), c->scratch, count * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return cfail(QSIM_ERR_DEVICE, "copy back failed");
    if (memcmp(a.data(), b.data(), count * 8) != 0) return cfail(QSIM_ERR_DEVICE, "RCCL loopback: received data differs");
    return QSIM_OK;
}

// ---- a plan's local steps on this rank's shard ------------------------------------------------------------------------------
extern "C" int qsim_shard_plan_apply_local(const qsim_shard_plan *p, int step, int shard, qsim_state *s) {
    if (!p || !s || step < 0 || step >= (int)p->plan.steps.size() || shard < 0 || shard >= p->P) return cfail(QSIM_ERR_ARG, "bad argument");
    const Step &st = p->plan.steps[step];
    if (st.exchange) return cfail(QSIM_ERR_ARG, "step %d is an exchange", step);
    return apply_ops(s, st.per_shard[shard]);
}

static void add(qsim_tune_report &total, const qsim_tune_report &r) {
    total.tile_passes += r.tile_passes; total.already_known += r.already_known; total.passes_tuned += r.passes_tuned;
    total.passes_reordered += r.passes_reordered; total.candidates_timed += r.candidates_timed;
    total.ms_ascending += r.ms_ascending; total.ms_best += r.ms_best; total.seconds += r.seconds;
}

// Planning of one shard's local steps: for each, the support the shard will have there (0 at the start on the shard that holds
// index 0; after an exchange what roles_of says; a shard that holds nothing is skipped) and the schedule choice / geometry
// tuning for exactly that situation.
static int plan_shard_steps(const Plan &plan, int shard, qsim_state *s, int max_candidates, double budget_ms, qsim_tune_report &total) {
    const int locals = plan.local_steps();
    SupportWalk walk(plan.m, shard, 1);
    for (const Step &st : plan.steps) {
        if (st.exchange) { walk.after_exchange(st); continue; }
        if (!walk.holds[0]) continue;
        qsim_circuit *c = nullptr;
        int rc = step_circuit(st.per_shard[(size_t)shard], plan.m, &c);
        qsim_tune_report r{};
        if (rc == QSIM_OK) {
            if (max_candidates > 1) rc = qsim_tune_circuit_support(s, c, max_candidates, budget_ms > 0 ? budget_ms / locals : 0.0, &r, walk.sup[0]);
            else rc = qsim_choose_schedule_for(s, c, walk.sup[0]);
        }
        qsim_circuit_free(c);
        if (rc) return cfail(rc, "%s", qsim_last_error());
        add(total, r);
        walk.sup[0] = ~0ULL; // a local step leaves the shard dense (its passes cover every qubit, or nearly: the engine knows better, the key then simply misses)
    }
    return QSIM_OK;
}

// Geometry planning for a shard's part of a plan: every local step's ops for `shard` as a circuit through
// qsim_tune_circuit (include/qsim.h, "measured pass geometry").  Leaves `s` reset; budget_ms bounds the total.
extern "C" int qsim_shard_plan_tune(const qsim_shard_plan *p, int shard, qsim_state *s, int max_candidates, double budget_ms,
                                    qsim_tune_report *report) {
    if (!p || !s || shard < 0 || shard >= p->P) return cfail(QSIM_ERR_ARG, "bad argument");
    qsim_tune_report total{};
    const int rc = plan_shard_steps(p->plan, shard, s, max_candidates < 2 ? 2 : max_candidates, budget_ms, total);
    if (rc) return rc;
    if (report) *report = total;
    return QSIM_OK;
}
