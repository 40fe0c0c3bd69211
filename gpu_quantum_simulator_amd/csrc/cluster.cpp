// cluster.cpp — sharded state vector inside ONE process: P = 2^p shards, each a qsim_state on some device (the same device
// may appear several times: "virtual shards", used to validate the sharded path where fewer than P GPUs exist).  The plan
// it runs and the helpers it shares with the one-process-per-GPU driver are shard_plan.h's.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "qsim_internal.h"
#include "shard_exec.h"

using namespace shard;

// How blocks travel, decided once by where the shards are: every shard on its own device -> RCCL (one ncclGroup of sends +
// recvs per exchange, on the shard streams); every shard on the SAME device (virtual shards) -> the pack kernel writes its
// blocks straight into the members' spare buffers and the buffers change roles; anything else -> pack + device-to-device copies.
enum class Transport { none, rccl, direct, copies };
constexpr int kMaxDirectBits = 3; // the pack kernel writes into the buffers of at most 2^3 members: a larger exchange of a `direct` cluster goes by copies

struct qsim_cluster {
    int n = 0, p = 0, m = 0, P = 0;
    std::vector<int> devices;
    std::vector<qsim_state *> shard;
    std::vector<double2 *> scratch;
    std::vector<int> pos; // logical -> physical after the last run
    uint64_t exchanges = 0;
    double exchange_bytes = 0;       // per shard, summed over exchanges, if every block travelled (the dense figure)
    double exchange_bytes_moved = 0; // what the shards together really sent (blocks of and for empty shards stay home)
    Transport transport = Transport::none;
    std::vector<ncclComm_t> comms;
    bool same_device = false;
    // same_device: the shards' state buffers are slices of ONE allocation and their scratch buffers slices of another, so
    // "block b of member j's new contents" is an index of the scratch pool and the re-layout of an exchange is a permutation
    // of index bits across the whole pool (qsim_flush_pack) — the last tile pass before an exchange writes straight there.
    char *pool[2] = {nullptr, nullptr};
    int state_pool = 0; // which pool the states are in (exchanges flip it)
    // the plan of the last circuit: a loop that runs one circuit again and again plans it once (compared gate by gate, not hashed)
    std::vector<LGate> planned_gates;
    Plan planned;
    int planned_tail = -1;
    PackCounts packs;
    std::vector<hipEvent_t> packed; // per shard: its pack of the current exchange has finished
    // A plan is only right from |0...0>: its first qubit placement is free BECAUSE that state is permutation-symmetric, and its
    // exchanges leave out what is zero from there (Step::mixed_*).  Set by qsim_cluster_reset, cleared when a circuit starts.
    bool fresh = false;
};

extern "C" const char *qsim_cluster_error(void) { return g_derr.c_str(); }

extern "C" void qsim_cluster_destroy(qsim_cluster *c) {
    if (!c) return;
    for (size_t r = 0; r < c->shard.size(); r++) (void)qsim_sync(c->shard[r]);
    for (ncclComm_t comm : c->comms) (void)ncclCommDestroy(comm);
    for (size_t r = 0; r < c->shard.size(); r++) {
        (void)hipSetDevice(c->devices[r]);
        if (r < c->packed.size() && c->packed[r]) (void)hipEventDestroy(c->packed[r]);
        if (c->scratch[r] && !c->pool[0]) (void)hipFree(c->scratch[r]);
        qsim_destroy(c->shard[r]);
    }
    for (char *pl : c->pool)
        if (pl) (void)hipFree(pl);
    delete c;
}

extern "C" int qsim_cluster_create(qsim_cluster **out, int num_q, int num_shards, const int *devices) {
    if (!out) return cfail(QSIM_ERR_ARG, "out is NULL");
    *out = nullptr;
    int p = 0;
    if (int rc = check_shards(num_q, num_shards, &p)) return rc;
    const int ndev = qsim_device_count();
    if (ndev <= 0) return cfail(QSIM_ERR_DEVICE, "no HIP device available (libqsim has no CPU fallback)");
    qsim_cluster *c = new qsim_cluster();
    c->n = num_q; c->p = p; c->m = num_q - p; c->P = num_shards;
    c->pos.resize(num_q);
    for (int q = 0; q < num_q; q++) c->pos[q] = q;
    bool one_device = p > 0;
    for (int r = 0; r < num_shards; r++) {
        const int dev = devices ? devices[r] : (r % ndev);
        if (dev < 0 || dev >= ndev) { qsim_cluster_destroy(c); return cfail(QSIM_ERR_ARG, "device %d out of range", dev); }
        c->devices.push_back(dev);
        one_device = one_device && dev == c->devices[0];
    }
    if (one_device) { // virtual shards: two pools, see qsim_cluster::pool
        (void)hipSetDevice(c->devices[0]);
        for (int i = 0; i < 2; i++)
            if (hipMalloc((void **)&c->pool[i], (size_t)16 << num_q) != hipSuccess) {
                (void)hipGetLastError();
                qsim_cluster_destroy(c);
                return cfail(QSIM_ERR_ALLOC, "Malloc error");
            }
    }
    for (int r = 0; r < num_shards; r++) {
        const int dev = c->devices[r];
        qsim_state *s = nullptr;
        int rc = c->pool[0] ? qsim_create_external(&s, c->m, dev, c->pool[0] + ((size_t)r * 16 << c->m)) : qsim_create(&s, c->m, dev);
        c->shard.push_back(s);
        if (rc == QSIM_OK) rc = qsim_set_option(s, QSIM_OPT_DEFER_FLIPS, 0); // a shard's last pass may have to do an exchange's re-layout
        c->scratch.push_back(c->pool[1] ? (double2 *)(c->pool[1] + ((size_t)r * 16 << c->m)) : nullptr);
        if (rc == QSIM_OK && p > 0 && !c->pool[0]) {
            (void)hipSetDevice(dev);
            if (hipMalloc((void **)&c->scratch[r], (size_t)16 << c->m) != hipSuccess) rc = QSIM_ERR_ALLOC;
        }
        if (rc != QSIM_OK) {
            const std::string msg = rc == QSIM_ERR_ALLOC ? "Malloc error" : qsim_last_error();
            qsim_cluster_destroy(c);
            return cfail(rc, "shard %d: %s", r, msg.c_str());
        }
    }
    // let every device reach its peers directly where the platform allows it
    for (int a = 0; a < num_shards; a++)
        for (int b = 0; b < num_shards; b++)
            if (c->devices[a] != c->devices[b]) {
                int can = 0;
                (void)hipSetDevice(c->devices[a]);
                if (hipDeviceCanAccessPeer(&can, c->devices[a], c->devices[b]) == hipSuccess && can)
                    (void)hipDeviceEnablePeerAccess(c->devices[b], 0); // "already enabled" is fine
            }
    (void)hipGetLastError();
    if (p > 0) {
        bool same = true, distinct = true;
        for (int a = 0; a < num_shards; a++)
            for (int b = a + 1; b < num_shards; b++) {
                if (c->devices[a] == c->devices[b]) distinct = false;
                else same = false;
            }
        c->same_device = same;
        c->transport = distinct ? Transport::rccl : same ? Transport::direct : Transport::copies;
        c->packed.assign((size_t)num_shards, nullptr);
        for (int r = 0; r < num_shards; r++) {
            (void)hipSetDevice(c->devices[r]);
            if (hipEventCreateWithFlags(&c->packed[r], hipEventDisableTiming) != hipSuccess) {
                qsim_cluster_destroy(c);
                return cfail(QSIM_ERR_DEVICE, "event creation failed");
            }
        }
        if (distinct) { // one RCCL communicator per device, all in this process
            c->comms.assign((size_t)num_shards, nullptr);
            const ncclResult_t nr = ncclCommInitAll(c->comms.data(), num_shards, c->devices.data());
            if (nr != ncclSuccess) {
                c->comms.clear();
                qsim_cluster_destroy(c);
                return cfail(QSIM_ERR_DEVICE, "ncclCommInitAll failed: %s", ncclGetErrorString(nr));
            }
            // A shard's scratch is touched by its own stream only in this mode (pack, then the sends): idle during local
            // steps, so it doubles as the second buffer of the shard's out-of-place tile passes (QSIM_OPT_PINGPONG).
            for (int r = 0; r < num_shards; r++) (void)qsim_set_spare_buffer(c->shard[r], c->scratch[r]);
        }
    }
    *out = c;
    return QSIM_OK;
}

extern "C" int qsim_cluster_num_shards(const qsim_cluster *c) { return c ? c->P : -1; }
extern "C" qsim_state *qsim_cluster_shard(qsim_cluster *c, int r) { return (c && r >= 0 && r < c->P) ? c->shard[r] : nullptr; }

extern "C" int qsim_cluster_set_option(qsim_cluster *c, int option, long value) {
    if (!c) return cfail(QSIM_ERR_ARG, "NULL cluster");
    for (qsim_state *s : c->shard) {
        const int rc = qsim_set_option(s, option, value);
        if (rc) return cfail(rc, "%s", qsim_last_error());
    }
    return QSIM_OK;
}

// Resets every shard to its part of |0...0> and the map to the identity.
extern "C" int qsim_cluster_reset(qsim_cluster *c) {
    if (!c) return cfail(QSIM_ERR_ARG, "NULL cluster");
    for (int r = 0; r < c->P; r++) {
        const int rc = qsim_reset_shard(c->shard[r], r == 0);
        if (rc) return cfail(rc, "%s", qsim_last_error());
    }
    for (int q = 0; q < c->n; q++) c->pos[q] = q;
    c->fresh = true;
    return QSIM_OK;
}

// flush: launch every shard's passes now.  The local step in front of an exchange leaves them queued: the exchange flushes
// them itself, so that the last tile pass can do the exchange's re-layout (qsim_flush_pack).
static int apply_local(qsim_cluster *c, const Step &st, bool flush) {
    for (int r = 0; r < c->P; r++) {
        if (int rc = apply_ops(c->shard[r], st.per_shard[r])) return rc;
        const int rc = flush ? qsim_flush(c->shard[r]) : QSIM_OK; // every shard's passes are in flight before the next one is scheduled
        if (rc) return cfail(rc, "%s", qsim_last_error());
    }
    return QSIM_OK;
}

static std::vector<Roles> all_roles(const qsim_cluster *c, const Step &st) {
    std::vector<Roles> roles;
    for (int r = 0; r < c->P; r++) roles.push_back(roles_of(r, c->m, st));
    return roles;
}

// Same device for every shard: shard r's pack writes block j of its new layout straight into the spare buffer of group
// member j (at block position mine(r)), then every shard takes its spare buffer — now complete — as its state.  One
// kernel per shard and no copy stage; ordering is by events between the shard streams, the host never waits.
static int exchange_direct(qsim_cluster *c, const Step &st) {
    const int k = (int)st.J.size();
    const std::vector<Roles> roles = all_roles(c, st);
    char *out_pool = c->pool[1 - c->state_pool];
    int to[kMaxDirectBits] = {0, 0, 0};
    uint32_t jmask = 0;
    for (int j = 0; j < k; j++) { to[j] = c->m + st.J[j]; jmask |= 1u << st.J[j]; }
    for (int r = 0; r < c->P; r++) {
        const Roles &ro = roles[(size_t)r];
        // destination of this shard's amplitudes inside the scratch pool: shard id = its own with the J bits replaced by the
        // amplitude's Lsel bits (to[]), block `mine` of that shard, the other local bits closed up below
        const uint64_t konst = ((uint64_t)((uint32_t)r & ~jmask) << c->m) | ((uint64_t)ro.mine << (c->m - k));
        if (int rc = pack_or_flush(c->shard[r], st, ro, to, konst, out_pool, c->packs)) return rc;
        c->exchange_bytes_moved += (double)blk_bytes(c->m, k) * __builtin_popcount(ro.send); // 0 from a shard that holds nothing
        if (hipEventRecord(c->packed[r], (hipStream_t)qsim_stream(c->shard[r])) != hipSuccess) return cfail(QSIM_ERR_DEVICE, "event record failed");
    }
    // every stream waits for every pack: the members' packs filled this shard's new buffer, and nobody may write into a
    // buffer (next exchange) that a straggler still reads
    for (int r = 0; r < c->P; r++)
        for (int o = 0; o < c->P; o++)
            if (o != r && hipStreamWaitEvent((hipStream_t)qsim_stream(c->shard[r]), c->packed[o], 0) != hipSuccess)
                return cfail(QSIM_ERR_DEVICE, "stream wait failed");
    for (int r = 0; r < c->P; r++) {
        void *buf = c->scratch[r];
        int rc = qsim_swap_buffer(c->shard[r], &buf);
        if (rc == QSIM_OK) rc = settle(c->shard[r], roles[(size_t)r]);
        if (rc) return cfail(rc, "%s", qsim_last_error());
        c->scratch[r] = (double2 *)buf;
    }
    c->state_pool = 1 - c->state_pool;
    return QSIM_OK;
}

// One device per shard: RCCL.  Every shard packs into its own scratch; then ONE group holds, for every shard, the
// 2^k - 1 sends of its scratch blocks and the 2^k - 1 receives into its state buffer, each pair of shards on its own
// xGMI link (k = 1: the pairwise half-shard exchange; k = log2 P: an all-to-all over all P - 1 links at once).
// Everything is stream-ordered on the shard streams (pack -> send/recv -> the next pass); the host does not wait.
static int exchange_rccl(qsim_cluster *c, const Step &st) {
    const int k = (int)st.J.size();
    const std::vector<Roles> roles = all_roles(c, st);
    for (int r = 0; r < c->P; r++)
        if (int rc = pack_or_flush(c->shard[r], st, roles[(size_t)r], nullptr, 0, c->scratch[r], c->packs)) return rc;
    std::vector<void *> state((size_t)c->P);
    for (int r = 0; r < c->P; r++) state[(size_t)r] = qsim_state_buffer(c->shard[r]);
    ncclResult_t nr = ncclGroupStart();
    for (int r = 0; r < c->P && nr == ncclSuccess; r++) {
        (void)hipSetDevice(c->devices[r]);
        nr = post_transfers(c->shard[r], roles[(size_t)r], k, c->scratch[r], state[(size_t)r], c->comms[r]);
        c->exchange_bytes_moved += (double)blk_bytes(c->m, k) * __builtin_popcount(roles[(size_t)r].send);
    }
    const ncclResult_t ne = ncclGroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return cfail(QSIM_ERR_DEVICE, "RCCL exchange failed: %s", ncclGetErrorString(nr));
    for (int r = 0; r < c->P; r++) { // the block a shard keeps
        (void)hipSetDevice(c->devices[r]);
        if (int rc = keep_own_and_settle(c->shard[r], roles[(size_t)r], k, c->scratch[r], state[(size_t)r])) return rc;
    }
    return QSIM_OK;
}

// Mixed placements (some shards share a device, some do not): pack, then device-to-device copies of the blocks.
static int exchange_copies(qsim_cluster *c, const Step &st) {
    const int k = (int)st.J.size();
    const size_t blk = blk_bytes(c->m, k);
    for (int r = 0; r < c->P; r++) {
        const int rc = qsim_pack_bits(c->shard[r], st.Lsel.data(), k, c->scratch[r]);
        if (rc) return cfail(rc, "%s", qsim_last_error());
    }
    for (int r = 0; r < c->P; r++) {
        const int rc = qsim_sync(c->shard[r]);
        if (rc) return cfail(rc, "%s", qsim_last_error());
    }
    // state block b of shard r  <-  scratch block mine(r) of group member b
    for (int r = 0; r < c->P; r++) {
        int mine;
        std::vector<int> members;
        peers_of(r, st.J, mine, members);
        char *dst = (char *)qsim_device_ptr(c->shard[r]);
        hipStream_t stream = (hipStream_t)qsim_stream(c->shard[r]);
        (void)hipSetDevice(c->devices[r]);
        for (int b = 0; b < (1 << k); b++) {
            const int peer = members[b];
            const char *src = (const char *)c->scratch[peer] + (size_t)mine * blk;
            hipError_t e;
            if (c->devices[peer] == c->devices[r])
                e = hipMemcpyAsync(dst + (size_t)b * blk, src, blk, hipMemcpyDeviceToDevice, stream);
            else
                e = hipMemcpyPeerAsync(dst + (size_t)b * blk, c->devices[r], src, c->devices[peer], blk, stream);
            if (e != hipSuccess) return cfail(QSIM_ERR_DEVICE, "exchange copy failed: %s", hipGetErrorString(e));
        }
    }
    for (int r = 0; r < c->P; r++) {
        const int rc = qsim_sync(c->shard[r]);
        if (rc) return cfail(rc, "%s", qsim_last_error());
    }
    c->exchange_bytes_moved += (double)blk * ((1 << k) - 1) * c->P; // every block travels: nothing is known to be zero on this path
    return QSIM_OK;
}

static int exchange(qsim_cluster *c, const Step &st) {
    const int k = (int)st.J.size();
    // a backstop: check_shards lets no cluster have groups this large, whatever the transport (the text dates from when only RCCL was checked)
    if (k > kMaxRoleBits) return cfail(QSIM_ERR_ARG, "exchange of %d qubits: groups of more than %d shards are not supported on RCCL", k, 1 << kMaxRoleBits);
    const Transport via = c->transport == Transport::direct && k > kMaxDirectBits ? Transport::copies : c->transport;
    const int rc = via == Transport::rccl ? exchange_rccl(c, st) : via == Transport::direct ? exchange_direct(c, st) : exchange_copies(c, st);
    if (rc) return rc;
    c->exchanges++;
    c->exchange_bytes += (double)blk_bytes(c->m, k) * ((1 << k) - 1);
    return QSIM_OK;
}

extern "C" const char *qsim_cluster_exchange_mode(const qsim_cluster *c) {
    static const char *const names[] = {"none", "rccl", "direct", "copies"};
    return names[(int)(c ? c->transport : Transport::none)];
}

// The plan of `circ` on this cluster, made now or kept from the last call when it was the same circuit.
static int cluster_plan_for(qsim_cluster *c, const qsim_circuit *circ) {
    if (int rc = check_shardable(circ, c->n, "clusters")) return rc;
    std::vector<LGate> gates;
    gates_of(circ, gates);
    bool same = c->planned_tail == tail_limit() && gates.size() == c->planned_gates.size();
    for (size_t i = 0; same && i < gates.size(); i++) {
        const LGate &a = gates[i], &b = c->planned_gates[i];
        same = a.kind == b.kind && a.q0 == b.q0 && a.q1 == b.q1 && (a.kind != QSIM_GATE_U1 || memcmp(a.m, b.m, sizeof a.m) == 0);
    }
    if (!same) {
        c->planned = Plan();
        c->planned_tail = -1;
        if (!build_plan(c->n, c->p, gates, c->planned)) return cfail(QSIM_ERR_ARG, "planner made no progress");
        c->planned_gates.swap(gates);
        c->planned_tail = tail_limit();
    }
    return QSIM_OK;
}

// Plans and runs ONE circuit from |0...0> (compute_state_vector semantics, quantum_simulator.c:115-254: one circuit per
// state): qsim_cluster_reset must come first.  The plan depends on it twice — the first qubit placement moves no data because
// |0...0> is permutation-symmetric, and the exchanges neither send nor read what is still zero (Step::mixed_*, roles_of) — so
// a second circuit on top of the first one's result is refused instead of silently dropping amplitudes.  What is checked is
// that no circuit has run since the reset (`fresh`) and that the map is the identity; a state the caller wrote through
// qsim_cluster_shard() after the reset is NOT noticed.
extern "C" int qsim_cluster_run_circuit(qsim_cluster *c, const qsim_circuit *circ) {
    if (!c || !circ) return cfail(QSIM_ERR_ARG, "NULL argument");
    // refused here, before the cluster stops being fresh; check_shardable in cluster_plan_for repeats it for qsim_cluster_plan
    if (circ->num_q != c->n) return cfail(QSIM_ERR_ARG, "circuit has %d qubits, cluster has %d", circ->num_q, c->n);
    if (!c->fresh) return cfail(QSIM_ERR_ARG, "cluster does not hold |0...0>: qsim_cluster_run_circuit runs one circuit per reset (call qsim_cluster_reset first)");
    for (int q = 0; q < c->n; q++)
        if (c->pos[q] != q) return cfail(QSIM_ERR_ARG, "cluster already holds a permuted state: reset it first");
    c->fresh = false;
    if (int rc = cluster_plan_for(c, circ)) return rc;
    const Plan &plan = c->planned;
    for (size_t i = 0; i < plan.steps.size(); i++) {
        const Step &st = plan.steps[i];
        const bool before_exchange = i + 1 < plan.steps.size() && plan.steps[i + 1].exchange;
        const int rc = st.exchange ? exchange(c, st) : apply_local(c, st, !before_exchange);
        if (rc) return rc;
    }
    c->pos = plan.final_pos;
    return QSIM_OK;
}

// Schedule choice (and, with max_candidates > 1, timing) for every shard's every local step, step by step for all shards, so
// that each exchange can be told what its senders' engines will actually have written by then: a schedule chosen here may
// leave other qubits untouched than the default one the planner assumed, and the last tile pass in front of an exchange does
// the re-layout itself only when what it writes covers what the receivers look at (Step::mixed_local).  Both masks bound
// the same state, so their intersection does too; holders and supports after the exchange follow from it.
extern "C" int qsim_cluster_plan(qsim_cluster *c, const qsim_circuit *circ, int max_candidates, double budget_ms) {
    if (!c || !circ) return cfail(QSIM_ERR_ARG, "NULL argument");
    int rc = cluster_plan_for(c, circ);
    if (rc) return rc;
    Plan &plan = c->planned;
    const int locals = plan.local_steps();
    const double budget_each = budget_ms > 0 && locals > 0 ? budget_ms / c->P / locals : 0.0;
    SupportWalk walk(plan.m, 0, c->P);
    for (Step &st : plan.steps) {
        if (st.exchange) {
            uint64_t written = 0, ranks = 0;
            walk.held(written, ranks);
            st.mixed_local &= written;
            st.mixed_rank &= ranks;
            walk.after_exchange(st);
            continue;
        }
        for (int r = 0; r < c->P; r++) {
            if (!walk.holds[(size_t)r]) continue;
            uint64_t &sup = walk.sup[(size_t)r];
            qsim_circuit *sc = nullptr;
            rc = step_circuit(st.per_shard[(size_t)r], plan.m, &sc);
            if (rc == QSIM_OK) {
                qsim_tune_report rep{};
                if (max_candidates > 1) rc = qsim_tune_circuit_support(c->shard[r], sc, max_candidates, budget_each, &rep, sup);
                else rc = qsim_choose_schedule_for(c->shard[r], sc, sup);
            }
            if (rc == QSIM_OK) rc = qsim_support_after(c->shard[r], sc, sup, &sup);
            qsim_circuit_free(sc);
            if (rc) return cfail(rc, "%s", qsim_last_error());
        }
    }
    return qsim_cluster_reset(c);
}

extern "C" int qsim_cluster_sync(qsim_cluster *c) {
    if (!c) return cfail(QSIM_ERR_ARG, "NULL cluster");
    for (qsim_state *s : c->shard) {
        const int rc = qsim_sync(s);
        if (rc) return cfail(rc, "%s", qsim_last_error());
    }
    return QSIM_OK;
}

static uint64_t physical_index(const qsim_cluster *c, uint64_t logical) {
    uint64_t out = 0;
    for (int q = 0; q < c->n; q++) out |= ((logical >> q) & 1ULL) << c->pos[q];
    return out;
}

// Amplitudes by LOGICAL basis index (gathered one by one: meant for samples and small registers).
extern "C" int qsim_cluster_read(qsim_cluster *c, uint64_t first, uint64_t count, double *out) {
    if (!c || !out) return cfail(QSIM_ERR_ARG, "NULL argument");
    const uint64_t N = 1ULL << c->n;
    if (first > N || count > N - first) return cfail(QSIM_ERR_ARG, "read range outside the state");
    const uint64_t mmask = (1ULL << c->m) - 1ULL;
    if (c->p == 0 || count > 4096) { // bulk: pull whole shards once and permute on the host
        std::vector<std::vector<double>> host(c->P);
        for (int r = 0; r < c->P; r++) {
            host[r].resize((size_t)2 << c->m);
            const int rc = qsim_read(c->shard[r], 0, 1ULL << c->m, host[r].data());
            if (rc) return cfail(rc, "%s", qsim_last_error());
        }
        for (uint64_t i = 0; i < count; i++) {
            const uint64_t ph = physical_index(c, first + i);
            out[2 * i] = host[ph >> c->m][2 * (ph & mmask)];
            out[2 * i + 1] = host[ph >> c->m][2 * (ph & mmask) + 1];
        }
        return QSIM_OK;
    }
    for (uint64_t i = 0; i < count; i++) {
        const uint64_t ph = physical_index(c, first + i);
        const int rc = qsim_read(c->shard[ph >> c->m], ph & mmask, 1, out + 2 * i);
        if (rc) return cfail(rc, "%s", qsim_last_error());
    }
    return QSIM_OK;
}

// measurement() of quantum_simulator.c:270-283 on a sharded state, in LOGICAL index order (the order the reference's
// cumulative distribution runs in, whatever the qubit map of the last run left behind).  A logical block = the 2^12
// amplitudes that agree on logical bits >= 12.  On shard r it occupies the local positions holding logical bits < 12
// (lo_mask), at the base given by the local positions holding logical bits >= 12 (hi_mask); logical bits sitting on
// rank-id positions are fixed by r.  So every shard sums |a|^2 per block ON ITS DEVICE (qsim_block_prob_masked), the
// host adds the "P partial sums" of SURVEY 8f row 1 in shard order, and a draw fetches only its own block
// (qsim_gather_masked from the shards that hold a part of it).  Nothing else crosses PCIe: 2^(n-12) doubles per shard
// plus 64 KiB per distinct block drawn.
extern "C" int qsim_cluster_sample(qsim_cluster *c, const double *randoms, long shots, uint64_t *out) {
    if (!c || (shots > 0 && (!randoms || !out))) return cfail(QSIM_ERR_ARG, "NULL argument");
    constexpr int kBlockBits = 12;
    const int bb = c->n < kBlockBits ? c->n : kBlockBits;
    const uint64_t N = 1ULL << c->n, nblocks = N >> bb, bsize = 1ULL << bb;
    std::vector<int> inv(c->n); // physical bit -> logical qubit
    for (int q = 0; q < c->n; q++) inv[c->pos[q]] = q;
    uint64_t hi_mask = 0, lo_mask = 0; // local positions by the kind of logical bit they hold
    for (int b = 0; b < c->m; b++) (inv[b] >= bb ? hi_mask : lo_mask) |= 1ULL << b;
    std::vector<int> hi_pos, lo_pos; // ascending local positions = the order deposit() fills them in
    for (int b = 0; b < c->m; b++) (inv[b] >= bb ? hi_pos : lo_pos).push_back(b);
    // block id / in-block index contributed by the rank-id bits of shard r
    auto rank_part = [&](int r, uint64_t &blk_bits, uint64_t &in_bits) {
        blk_bits = in_bits = 0;
        for (int g = 0; g < c->p; g++) {
            const int L = inv[c->m + g];
            if ((r >> g) & 1) (L >= bb ? blk_bits : in_bits) |= 1ULL << (L >= bb ? L - bb : L);
        }
    };
    std::vector<double> prefix(nblocks, 0.0), part((size_t)1 << hi_pos.size());
    for (int r = 0; r < c->P; r++) {
        const int rc = qsim_block_prob_masked(c->shard[r], hi_mask, lo_mask, part.data());
        if (rc) return cfail(rc, "%s", qsim_last_error());
        uint64_t rb, ri;
        rank_part(r, rb, ri);
        for (uint64_t w = 0; w < part.size(); w++) {
            uint64_t blk = rb;
            for (size_t j = 0; j < hi_pos.size(); j++)
                if ((w >> j) & 1ULL) blk |= 1ULL << (inv[hi_pos[j]] - bb);
            prefix[blk] += part[w];
        }
    }
    double acc = 0.0;
    for (uint64_t b = 0; b < nblocks; b++) { acc += prefix[b]; prefix[b] = acc; } // cumulative at the END of block b
    std::vector<double> blk(2 * bsize), piece((size_t)2 << lo_pos.size());
    uint64_t cached = ~0ULL;
    auto fetch_block = [&](uint64_t b) -> int {
        for (int r = 0; r < c->P; r++) {
            uint64_t rb, ri;
            rank_part(r, rb, ri);
            uint64_t gmask = 0; // block-id bits decided by rank-id positions
            for (int g = 0; g < c->p; g++)
                if (inv[c->m + g] >= bb) gmask |= 1ULL << (inv[c->m + g] - bb);
            if ((b & gmask) != rb) continue; // this shard holds no part of block b
            uint64_t base = 0;
            for (size_t j = 0; j < hi_pos.size(); j++)
                if ((b >> (inv[hi_pos[j]] - bb)) & 1ULL) base |= 1ULL << hi_pos[j];
            const int rc = qsim_gather_masked(c->shard[r], base, lo_mask, piece.data());
            if (rc) return cfail(rc, "%s", qsim_last_error());
            for (uint64_t i = 0; i < ((uint64_t)1 << lo_pos.size()); i++) {
                uint64_t in = ri;
                for (size_t j = 0; j < lo_pos.size(); j++)
                    if ((i >> j) & 1ULL) in |= 1ULL << inv[lo_pos[j]];
                blk[2 * in] = piece[2 * i];
                blk[2 * in + 1] = piece[2 * i + 1];
            }
        }
        return QSIM_OK;
    };
    for (long k = 0; k < shots; k++) {
        const double rnd = randoms[k];
        uint64_t lo = 0, hi = nblocks;
        while (lo < hi) { // first block whose end value is non-zero and >= r (quantum_simulator.c:279)
            const uint64_t mid = (lo + hi) >> 1;
            if (prefix[mid] == 0.0 || prefix[mid] < rnd) lo = mid + 1;
            else hi = mid;
        }
        uint64_t idx = N - 1;
        bool found = false;
        for (uint64_t b = lo; b < nblocks && !found; b++) {
            if (b != cached) {
                const int rc = fetch_block(b);
                if (rc) return rc;
                cached = b;
            }
            double cum = b ? prefix[b - 1] : 0.0;
            for (uint64_t i = 0; i < bsize; i++) {
                cum += blk[2 * i] * blk[2 * i] + blk[2 * i + 1] * blk[2 * i + 1];
                if (!(cum == 0.0 || cum < rnd)) { idx = b * bsize + i; found = true; break; }
            }
        }
        out[k] = idx;
    }
    return QSIM_OK;
}

extern "C" int qsim_cluster_norm2(qsim_cluster *c, double *out) {
    if (!c || !out) return cfail(QSIM_ERR_ARG, "NULL argument");
    double tot = 0;
    for (qsim_state *s : c->shard) {
        double v = 0;
        const int rc = qsim_norm2(s, &v);
        if (rc) return cfail(rc, "%s", qsim_last_error());
        tot += v;
    }
    *out = tot;
    return QSIM_OK;
}

// What the two Pauli entry points open with: the argument checks of every Pauli entry point (`third`: the results or the angles;
// `thetas`: the angles, where there are any), then every mask mapped from logical qubits through `pos` into X and Z, and the refusal
// to pair shards across devices.
static int physical_terms(qsim_cluster *c, const char *who, const uint64_t *x_masks, const uint64_t *z_masks, const void *third, const double *thetas,
                          long num_terms, std::vector<uint64_t> &X, std::vector<uint64_t> &Z) {
    if (!c) return cfail(QSIM_ERR_ARG, "NULL cluster");
    if (const int rc = qsim::check_pauli_terms(cfail, who, c->n, x_masks, z_masks, third, thetas, num_terms)) return rc;
    X.resize((size_t)num_terms), Z.resize((size_t)num_terms);
    for (long t = 0; t < num_terms; t++) {
        X[(size_t)t] = physical_index(c, x_masks[t]);
        Z[(size_t)t] = physical_index(c, z_masks[t]);
        if ((X[(size_t)t] >> c->m) != 0 && !c->same_device)
            return cfail(QSIM_ERR_ARG,
                         "%s: term %ld has X or Y on a qubit that currently selects the shard, and the shards are on "
                         "different devices: reading a partner shard across devices is not implemented",
                         who, t);
    }
    return QSIM_OK;
}
// x_rank pairs shard r with shard r ^ xr: the member with the highest bit of xr clear does the pair's work, the other one nothing
static bool sweeps_pair(int r, uint64_t xr) { return (((uint64_t)r >> (63 - __builtin_clzll(xr))) & 1ULL) == 0; }

// <psi|P_t|psi> on the sharded state.  Masks arrive in logical qubits; mapped through `pos` they split into local index bits
// (< m) and shard-id bits.  Z on shard-id bits is a sign per shard.  X on shard-id bits (x_rank) pairs shard r with shard
// r ^ x_rank: over the whole register the sum runs over the indices with the highest bit of x clear, and that bit is then a
// shard-id bit — so the shard of each pair that has it clear sweeps ALL its local indices against its partner's buffer, and
// the other one does nothing.  With x_rank == 0 every shard sweeps its own half (highest LOCAL bit of x clear).  Either way
// every amplitude is read once.  A partner buffer is only readable in place when both shards are on one device.
extern "C" int qsim_cluster_expect_paulis(qsim_cluster *c, const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, double *out) {
    std::vector<uint64_t> X, Z;
    if (const int rc = physical_terms(c, "qsim_cluster_expect_paulis", x_masks, z_masks, out, nullptr, num_terms, X, Z)) return rc;
    if (num_terms == 0) return QSIM_OK;
    // a shard's buffer is about to be read from another shard's stream: everything queued must have run, lazily held states
    // must have been written
    for (qsim_state *s : c->shard)
        if (!qsim_device_ptr(s) || qsim_sync(s) != QSIM_OK) return cfail(QSIM_ERR_DEVICE, "%s", qsim_last_error());
    // terms by x_rank, in order of first appearance
    std::vector<uint64_t> ranks_x;
    for (long t = 0; t < num_terms; t++)
        if (std::find(ranks_x.begin(), ranks_x.end(), X[(size_t)t] >> c->m) == ranks_x.end()) ranks_x.push_back(X[(size_t)t] >> c->m);
    for (long t = 0; t < num_terms; t++) out[t] = 0.0;
    std::vector<uint64_t> gx, gz;
    std::vector<long> gt;
    std::vector<double> part;
    for (int r = 0; r < c->P; r++)
        for (const uint64_t xr : ranks_x) {
            if (xr != 0 && !sweeps_pair(r, xr)) continue; // its partner counts the pair
            gx.clear(), gz.clear(), gt.clear();
            for (long t = 0; t < num_terms; t++)
                if ((X[(size_t)t] >> c->m) == xr) gx.push_back(X[(size_t)t]), gz.push_back(Z[(size_t)t]), gt.push_back(t);
            part.assign(gt.size(), 0.0);
            const void *partner = xr ? qsim_state_buffer(c->shard[(size_t)((uint64_t)r ^ xr)]) : nullptr;
            const int rc = qsim::expect_paulis_shard(c->shard[(size_t)r], partner, (uint64_t)r, gx.data(), gz.data(), (long)gt.size(), part.data());
            if (rc) return cfail(rc, "shard %d: %s", r, qsim_last_error());
            for (size_t i = 0; i < gt.size(); i++) out[gt[i]] += part[i];
        }
    return QSIM_OK;
}

// exp(-i theta/2 P_t) on the sharded state, t = 0 first (DESIGN "Pauli rotations").  Masks arrive in logical qubits and are mapped
// through `pos`, as in qsim_cluster_expect_paulis.  Z on shard-id bits is a sign per shard.  A run whose x has shard-id bits
// (x_rank) pairs shard r with shard r ^ x_rank: the member with the highest bit of x_rank clear sweeps all its local indices
// against its partner's buffer and writes both; the other member does nothing.  For that every shard has been settled and its
// stream waited for, and afterwards the partner's stream waits for the sweep that wrote its buffer.
extern "C" int qsim_cluster_apply_pauli_rotations(qsim_cluster *c, const uint64_t *x_masks, const uint64_t *z_masks, const double *thetas, long num_terms) {
    std::vector<uint64_t> X, Z;
    if (const int rc = physical_terms(c, "qsim_cluster_apply_pauli_rotations", x_masks, z_masks, thetas, thetas, num_terms, X, Z)) return rc;
    if (num_terms == 0) return QSIM_OK;
    const uint64_t mmask = qsim::index_mask(c->m);
    c->fresh = false; // the state is no longer |0...0>: a circuit needs a reset first
    uint64_t paired_by = 0; // the x_rank all shards are settled and waited for (0: not)
    for (const qsim::RotRoute &rt : qsim::route_rotations(X.data(), Z.data(), num_terms, mmask)) {
        const uint64_t x = X[(size_t)rt.first], xr = x >> c->m;
        if (rt.gate) {
            double U[8];
            qsim::pauli_rot_1q((Z[(size_t)rt.first] & x) != 0, thetas[rt.first], U);
            for (qsim_state *s : c->shard)
                if (const int rc = qsim_apply_1q(s, U, __builtin_ctzll(x))) return cfail(rc, "%s", qsim_last_error());
            paired_by = 0;
            continue;
        }
        if (xr == 0) {
            for (int r = 0; r < c->P; r++) {
                const int rc = qsim::pauli_rot_run(c->shard[(size_t)r], nullptr, (uint64_t)r, x, Z.data() + rt.first, thetas + rt.first, rt.count);
                if (rc) return cfail(rc, "shard %d: %s", r, qsim_last_error());
            }
            paired_by = 0;
            continue;
        }
        // a shard's buffer is about to be read and written from another shard's stream: everything queued must have run.  A pair
        // of which one member holds nothing gets that member's zeros written; a pair that holds nothing at all stays untouched.
        if (paired_by != xr)
            for (int r = 0; r < c->P; r++) {
                qsim_state *s = c->shard[(size_t)r];
                if (qsim_holds_nothing(s) && qsim_holds_nothing(c->shard[(size_t)((uint64_t)r ^ xr)])) continue;
                if (qsim_sync(s) != QSIM_OK) return cfail(QSIM_ERR_DEVICE, "shard %d: %s", r, qsim_last_error());
            }
        paired_by = xr;
        for (int r = 0; r < c->P; r++) {
            if (!sweeps_pair(r, xr)) continue; // its partner sweeps the pair
            qsim_state *s = c->shard[(size_t)r], *other = c->shard[(size_t)((uint64_t)r ^ xr)];
            if (qsim_holds_nothing(s) && qsim_holds_nothing(other)) continue;
            void *partner = qsim_state_buffer(other);
            if (!partner) return cfail(QSIM_ERR_DEVICE, "shard %d: %s", (int)((uint64_t)r ^ xr), qsim_last_error());
            const int rc = qsim::pauli_rot_run(s, partner, (uint64_t)r, x, Z.data() + rt.first, thetas + rt.first, rt.count);
            if (rc) return cfail(rc, "shard %d: %s", r, qsim_last_error());
            // the partner's stream must not run ahead of the sweep that wrote its buffer
            hipError_t e = hipEventRecord(c->packed[(size_t)r], (hipStream_t)qsim_stream(s));
            if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)qsim_stream(other), c->packed[(size_t)r], 0);
            if (e != hipSuccess) return cfail(QSIM_ERR_DEVICE, "shard %d: ordering the partner's stream failed: %s", r, hipGetErrorString(e));
        }
    }
    return QSIM_OK;
}

extern "C" int qsim_cluster_exchange_stats(const qsim_cluster *c, uint64_t *exchanges, double *bytes_per_shard) {
    if (!c) return QSIM_ERR_ARG;
    if (exchanges) *exchanges = c->exchanges;
    if (bytes_per_shard) *bytes_per_shard = c->exchange_bytes;
    return QSIM_OK;
}
extern "C" int qsim_cluster_exchange_bytes_moved(const qsim_cluster *c, double *bytes_all_shards) {
    if (!c || !bytes_all_shards) return QSIM_ERR_ARG;
    *bytes_all_shards = c->exchange_bytes_moved;
    return QSIM_OK;
}
extern "C" int qsim_cluster_pack_counts(const qsim_cluster *c, uint64_t *fused, uint64_t *separate) {
    if (!c) return QSIM_ERR_ARG;
    if (fused) *fused = c->packs.fused;
    if (separate) *separate = c->packs.separate;
    return QSIM_OK;
}
