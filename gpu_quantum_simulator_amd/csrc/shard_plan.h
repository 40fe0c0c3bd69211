// shard_plan.h — what the host files of the sharded path share: the plan of a circuit on P = 2^p shards, the roles of a shard in
// one exchange, and the few helpers both drivers execute a plan with.  New design — the reference is single-device.
//
// Physical index bits 0..m-1 (m = n - p) are local to a shard, bits m..n-1 are the shard id.  A host-side
// logical->physical qubit map decides what needs data movement:
//   * gates on local qubits run through the single-GPU engine on every shard;
//   * a diagonal gate on a global qubit is a per-shard scalar, a CX with global control and local target is an X on
//     the shards whose control bit is 1 — no communication;
//   * anything else on a global qubit waits; when nothing more can run, ONE exchange swaps k global qubits with k
//     local ones: k_pack lays every shard out as 2^k contiguous blocks, then block b of shard r goes to group
//     member b.  New globals = furthest next non-diagonal use (Belady); the first placement is free because
//     |0...0> is symmetric under qubit permutations.
// Who defines what:
//   shard_plan.cpp  the planner (build_plan and everything only it uses), roles_of / peers_of / gates_of, and the host-only part of
//                   the C ABI's qsim_shard_plan.  No RCCL and no HIP call: it is the C++ twin of tests/py_shard_plan.py.
//   shard_exec.cpp  the error channel (g_derr, cfail), the refusals both drivers share, a local step onto a state or into a
//                   circuit, and the RCCL leg of one shard's exchange (declared in shard_exec.h, which only the two drivers
//                   include: it needs <rccl/rccl.h>, and the planner file is kept free of it).
//   cluster.cpp     qsim_cluster: one process, P shards (the same device may appear several times: "virtual shards"), three
//                   exchange transports, reads, sampling, Pauli sums.
//   rank_comm.cpp   qsim_rank_comm: one process per GPU on RCCL, and the qsim_shard_plan functions that take a qsim_state.
#ifndef QSIM_SHARD_PLAN_H
#define QSIM_SHARD_PLAN_H

#include <complex>
#include <cstdint>
#include <string>
#include <vector>

#include "circuit.h"

namespace shard __attribute__((visibility("hidden"))) { // internal to libqsim: the library exports the C ABI only

using cd = std::complex<double>;

struct LGate { // logical gate
    int kind;  // QSIM_GATE_U1 / QSIM_GATE_CX
    int q0, q1;
    cd m[4];
    long idx = 0; // position in the circuit
    bool diag() const { return m[1] == cd(0, 0) && m[2] == cd(0, 0); }
};

enum class OpKind : int { u1 = 1, cx = 2, scale = 3 }; // the integers qsim_shard_plan_local_ops reports (include/qsim.h)
struct LocalOp { // per-shard op in local physical coordinates
    OpKind kind;
    int a, b;    // u1: qubit a; cx: a -> b
    cd m[4];     // u1: the matrix; scale: m[0] is the factor
};

// THE replay of a local step's ops.  A sink has cx(a, b), u1(m, a) and scale(z), each returning 0 or an error code that ends
// the replay; one that has no scalar multiply of its own takes the factor as a gate (scale_as_gate).
template <class Sink> int replay(const std::vector<LocalOp> &ops, Sink &&sink) {
    for (const LocalOp &o : ops) {
        const int rc = o.kind == OpKind::cx ? sink.cx(o.a, o.b) : o.kind == OpKind::u1 ? sink.u1(o.m, o.a) : sink.scale(o.m[0]);
        if (rc) return rc;
    }
    return 0;
}
// A per-shard factor is diag(z, z) on qubit 0.
template <class Sink> int scale_as_gate(Sink &sink, cd z) {
    const cd d[4] = {z, cd(0, 0), cd(0, 0), z};
    return sink.u1(d, 0);
}
inline const double *as_doubles(const cd *m) { return reinterpret_cast<const double *>(m); } // (re, im) pairs, as the C ABI takes matrices

struct Step {
    bool exchange = false;
    std::vector<int> J, Lsel;                    // exchange: shard-id bits and local positions, ascending, paired
    std::vector<std::vector<LocalOp>> per_shard; // local: ops for every shard
    // exchange: where the state can be non-zero just before it, as PHYSICAL bit sets (local positions / shard-id bits).  A run
    // starts from |0...0> (quantum_simulator.c:175-177) and a qubit stays |0> until a gate mixes it (a non-diagonal 1-qubit
    // gate, or a CX onto it whose control may be 1), so every amplitude with a 1 at a qubit outside this set is exactly
    // zero.  The same on every rank (it follows from the gate list alone), which is what lets an exchange leave out the
    // blocks of shards that hold nothing and lets the receivers keep visiting only the part of the shard that can be non-zero.
    uint64_t mixed_local = 0, mixed_rank = 0;
};

struct Plan {
    int n = 0, p = 0, m = 0;
    std::vector<Step> steps;
    std::vector<int> final_pos;
    int exchanges = 0;
    int tail_gates = 0; // gate statements handed on across an exchange (small_tail)
    double local_sweeps = 0; // predicted time of the local steps on their busiest shard, in sweeps of the shard (pass_time_cost)
    int local_steps() const {
        int c = 0;
        for (const Step &st : steps) c += !st.exchange;
        return c;
    }
};

// Who sends what in one exchange, for one rank, when only part of the register can be non-zero (Step::mixed_*).  A shard whose
// id has a 1 at a shard-id bit outside mixed_rank holds nothing; after the exchange the J bits of its id carry the qubits that
// sat at the local positions Lsel, so a shard is empty afterwards when one of THOSE is outside mixed_local.  Nothing travels
// from or to an empty shard, and a receiver's new contents can only be non-zero where the local index stays inside
// `new_support`: the surviving mixed local positions, moved down over the ones that left, plus the top k positions (the
// sender's member index) for the shard-id bits that were mixed.
struct Roles {
    int mine = 0;
    std::vector<int> members;
    bool empty_before = false, empty_after = false;
    uint32_t send = 0, recv = 0; // bit b: block b goes to / comes from members[b] (never bit `mine`)
    bool keep_own = false;       // block `mine` stays here and holds data
    uint32_t unread = 0;         // blocks of this rank's packed layout nobody looks at
    uint64_t new_support = 0;
};
// Roles::send / recv / unread and k_pack's skip mask have one bit per block: groups of at most 32 shards.  check_shards keeps
// every plan and cluster inside it, exchange() and rank_exchange refuse a larger k, roles_of asserts it.
constexpr int kMaxRoleBits = 5;
Roles roles_of(int rank, int m, const Step &st);
void peers_of(int rank, const std::vector<int> &J, int &mine, std::vector<int> &members);
inline size_t blk_bytes(int m, int k) { return ((size_t)16 << m) >> k; } // one of the 2^k blocks of a packed fp64 shard

// Which of the ranks first .. first + count - 1 hold anything, and where each one's state can be non-zero (local index bits),
// along the steps of a plan run from |0...0>: only shard 0 holds something at the start, every exchange deals the roles anew
// (roles_of), and a local step widens a holder's support by whatever its caller finds out (the planner by scheduling the
// step, a driver by asking the shard's engine).
struct SupportWalk {
    int m, first;
    std::vector<char> holds;
    std::vector<uint64_t> sup;
    SupportWalk(int m_, int first_, int count) : m(m_), first(first_), holds((size_t)count, 0), sup((size_t)count, 0) {
        if (first == 0) holds[0] = 1;
    }
    void held(uint64_t &local, uint64_t &ranks) const { // |= over the holders: where they can be non-zero, and their ids
        for (size_t i = 0; i < holds.size(); i++)
            if (holds[i]) { local |= sup[i]; ranks |= (uint64_t)first + i; }
    }
    void after_exchange(const Step &st) {
        for (size_t i = 0; i < holds.size(); i++) {
            const Roles ro = roles_of(first + (int)i, m, st);
            holds[i] = !ro.empty_after;
            sup[i] = ro.empty_after ? 0 : ro.new_support;
        }
    }
};

// The placement policies and hand-over limits are planned in full and the cheapest plan is kept (the comment at the definition).
bool build_plan(int n, int p, const std::vector<LGate> &gates, Plan &plan);
int tail_limit(); // QSIM_SHARD_TAIL, or the default: a plan is only reused under the limit it was made with
void gates_of(const qsim_circuit *c, std::vector<LGate> &out);

// ---- shard_exec.cpp ---------------------------------------------------------------------------------------------------------
// The error channel of the sharded path (qsim_cluster_error): sets the thread's message and returns `code`.
extern thread_local std::string g_derr;
int cfail(int code, const char *fmt, ...);
// num_shards = 2^p with at most 2^kMaxRoleBits shards of at least 2 qubits each, or QSIM_ERR_ARG.
int check_shards(int num_q, int num_shards, int *p);
// A circuit the planner takes: n_expected qubits (< 0: any number) and no generic 2-qubit gate; `where`: "clusters" / "shards".
int check_shardable(const qsim_circuit *circ, int n_expected, const char *where);
// The ops of a local step queued on a shard's state (a factor through qsim_scale), and as a circuit on its m local qubits.
int apply_ops(qsim_state *s, const std::vector<LocalOp> &ops);
int step_circuit(const std::vector<LocalOp> &ops, int m, qsim_circuit **out);
// What the shard's engine is told once the blocks of an exchange are in place.
int settle(qsim_state *s, const Roles &r);

} // namespace shard

struct qsim_shard_plan { // the plan as an object of the C ABI
    shard::Plan plan;
    int P = 0;
};

#endif
