// shard_plan.cpp — the planner of the sharded path and the host-only part of qsim_shard_plan (shard_plan.h says who owns what).
// Host code only: no device is touched, no HIP or RCCL call is made and no RCCL header is read here (scheduler.h, needed for the
// engine's own Scheduler, still reads qsim_internal.h and through it the HIP headers).  The planner is the C++ twin of
// distributed.ShardPlan's Python restatement in tests/py_shard_plan.py (tests compare the two step by step).
#include <algorithm>
#include <cassert>
#include <cstdlib>

#include "scheduler.h"
#include "shard_plan.h"

namespace shard {

void peers_of(int rank, const std::vector<int> &J, int &mine, std::vector<int> &members) {
    const int k = (int)J.size();
    mine = 0;
    int base = rank;
    for (int i = 0; i < k; i++) { mine |= ((rank >> J[i]) & 1) << i; base &= ~(1 << J[i]); }
    members.resize((size_t)1 << k);
    for (int b = 0; b < (1 << k); b++) {
        int r = base;
        for (int i = 0; i < k; i++) r |= ((b >> i) & 1) << J[i];
        members[b] = r;
    }
}

Roles roles_of(int rank, int m, const Step &st) {
    Roles r;
    const int k = (int)st.J.size();
    assert(k <= kMaxRoleBits); // one bit per block below; see kMaxRoleBits for who keeps k inside it
    peers_of(rank, st.J, r.mine, r.members);
    uint32_t jmask = 0, jin = 0, lin = 0;
    uint64_t lsel = 0;
    for (int i = 0; i < k; i++) {
        jmask |= 1u << st.J[i];
        lsel |= 1ULL << st.Lsel[i];
        if (st.mixed_rank >> st.J[i] & 1ULL) jin |= 1u << i;
        if (st.mixed_local >> st.Lsel[i] & 1ULL) lin |= 1u << i;
    }
    const bool base_ok = (((uint64_t)rank & ~(uint64_t)jmask) & ~st.mixed_rank) == 0;
    auto before = [&](int b) { return !base_ok || ((uint32_t)b & ~jin) != 0; }; // member b holds nothing before / after
    auto after = [&](int b) { return !base_ok || ((uint32_t)b & ~lin) != 0; };
    r.empty_before = before(r.mine);
    r.empty_after = after(r.mine);
    for (int b = 0; b < (1 << k); b++) {
        if (after(b)) r.unread |= 1u << b;
        if (b == r.mine) continue;
        if (!r.empty_before && !after(b)) r.send |= 1u << b;
        if (!r.empty_after && !before(b)) r.recv |= 1u << b;
    }
    r.keep_own = !r.empty_before && !r.empty_after;
    for (int b = 0; b < m; b++) {
        if (!(st.mixed_local >> b & 1ULL) || (lsel >> b & 1ULL)) continue;
        r.new_support |= 1ULL << (b - __builtin_popcountll(lsel & ((1ULL << b) - 1ULL)));
    }
    for (int i = 0; i < k; i++)
        if (jin >> i & 1u) r.new_support |= 1ULL << (m - k + i);
    return r;
}

void gates_of(const qsim_circuit *c, std::vector<LGate> &out) {
    out.reserve((size_t)c->count);
    for (long i = 0; i < c->count; i++) {
        const qsim_gate_rec &g = c->gates[i];
        LGate lg{};
        lg.kind = g.kind; lg.q0 = g.q0; lg.q1 = g.q1; lg.idx = i;
        if (g.kind == QSIM_GATE_U1)
            for (int k = 0; k < 4; k++) lg.m[k] = cd(c->mats2[8 * (long)g.mat + 2 * k], c->mats2[8 * (long)g.mat + 2 * k + 1]);
        out.push_back(lg);
    }
}

// QSIM_SHARD_TAIL: the largest last pass (in gate statements) that is handed on to the next segment; 0 = never (the plain
// "run everything that can run" planner, which tests/py_shard_plan.py restates).  An experiment override like QSIM_SCHED_*.
int tail_limit() {
    if (const char *v = getenv("QSIM_SHARD_TAIL")) return atoi(v);
    return 24;
}

namespace {

constexpr long kInf = 1L << 60;

// qubits this gate needs in LOCAL positions
void needs_local(const LGate &g, int out[2], int &cnt) {
    cnt = 0;
    if (g.kind == QSIM_GATE_CX) {
        if (g.q0 != g.q1) out[cnt++] = g.q1;
    } else if (!g.diag()) {
        out[cnt++] = g.q0;
    }
}

// local_only: candidates are the qubits that are local now, so an exchange swaps ALL p global qubits (k = p).  On a
// fully connected node a k-qubit swap sends 2^k - 1 blocks of 2^-k of the shard over as many links at once, so its
// time FALLS with k; whether the extra qubits it evicts come back too soon is what plan_cost decides.
std::vector<int> choose_globals(const std::vector<LGate> &gates, const std::vector<int> &pos, int n, int p, int m, bool local_only = false) {
    if (m < p) local_only = false; // fewer local qubits than global ones: nothing to choose from
    std::vector<long> nxt(n, kInf);
    int found = 0;
    for (size_t i = 0; i < gates.size() && found < n; i++) {
        int q[2], c;
        needs_local(gates[i], q, c);
        for (int k = 0; k < c; k++)
            if (nxt[q[k]] == kInf) { nxt[q[k]] = (long)i; found++; }
    }
    std::vector<int> order;
    for (int q = 0; q < n; q++)
        if (!local_only || pos[q] < m) order.push_back(q);
    // far next use first; then already-global (nothing to move); then a high position — same key as the Python twin
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        if (nxt[a] != nxt[b]) return nxt[a] > nxt[b];
        const bool ga = pos[a] >= m, gb = pos[b] >= m;
        if (ga != gb) return ga;
        return pos[a] > pos[b];
    });
    order.resize(p);
    return order;
}

// The ops of a shard's segment into the engine's scheduler, which has no scalar multiply: a factor goes in as a gate.
struct SchedSink {
    qsim::Scheduler &sched;
    int cx(int a, int b) { sched.add_cx(a, b); return 0; }
    int u1(const cd *m, int a) { sched.add_1q(m, a); return 0; }
    int scale(cd z) { return scale_as_gate(*this, z); }
};

// The gates of `run` (indices) that the engine's scheduler would put into the LAST pass of the segment, when that pass is
// a small one: the segment's gates are scheduled here exactly as a shard's engine will schedule them (same Scheduler, same
// settings; the shard-dependent ops in their busiest form: a CX controlled by a shard-id bit as an X), with every pass
// listing the gates it absorbed.  A segment ends where the next gate needs a qubit that is not local, not where a pass
// is full, so its last pass often carries a handful of gates and still costs a whole sweep over the shard — on every
// segment.  Those gates can just as well wait for the exchange: they come last in a valid order, and what they touch stays
// local (the planner evicts by furthest next use, and theirs is now the nearest).
std::vector<size_t> small_tail(const std::vector<LGate> &run, const std::vector<int> &pos, int m, bool from_reset, int max_gates) {
    std::vector<size_t> out;
    if (max_gates <= 0 || m < 12 || run.size() < 2) return out;
    qsim::SchedConfig cfg = qsim::engine_sched_config(m, 3, 12, 3, 32, 10, false, from_reset ? 0 : ~0ULL);
    cfg.track = 1;
    qsim::Scheduler sched(cfg);
    std::vector<size_t> which; // scheduler gate number -> index into run
    static const cd X[4] = {cd(0, 0), cd(1, 0), cd(1, 0), cd(0, 0)};
    for (size_t i = 0; i < run.size(); i++) {
        const LGate &g = run[i];
        if (g.kind == QSIM_GATE_CX) {
            if (g.q0 == g.q1) continue;
            if (pos[g.q0] < m) sched.add_cx(pos[g.q0], pos[g.q1]);
            else sched.add_1q(X, pos[g.q1]);
        } else if (pos[g.q0] < m) {
            sched.add_1q(g.m, pos[g.q0]);
        } else {
            continue; // a factor per shard
        }
        which.push_back(i);
    }
    std::vector<qsim::Pass> passes;
    sched.finish(passes);
    if (passes.size() < 2 || passes.back().kclass != QSIM_K_TILE) return out;
    const qsim::Pass &last = passes.back();
    if ((int)last.src.size() > max_gates) return out;
    for (uint32_t gi : last.src) out.push_back(which[gi]);
    std::sort(out.begin(), out.end());
    return out;
}

// Where a shard's state can be non-zero after a local step, as its engine will know it: the step's ops are scheduled exactly
// as qsim_flush will schedule them, and whatever lies outside (support before | the tile qubits of the passes) has not been
// touched since it was zero.  ANY valid schedule of the same ops gives a valid bound (the final state does not depend on the
// schedule), so it does not matter whether the engine later takes this very schedule or another variant of it; what matters
// is that every rank computes the same mask, which it does: same plan, same code.  Tighter than counting the qubits some
// non-diagonal gate has touched (x q; cx q,t; x q leaves q where it was, and the fused cluster shows it).
// cost_sweeps (optional): += what the step is predicted to take, in sweeps of the shard (pass_time_cost).
uint64_t scheduled_support(const std::vector<LocalOp> &ops, int m, uint64_t support, double *cost_sweeps = nullptr) {
    const uint64_t all = qsim::index_mask(m);
    if (ops.empty() || (!cost_sweeps && (support & all) == all)) return support & all;
    qsim::Scheduler sched(qsim::engine_sched_config(m, 3, 12, 3, 32, 10, false, (support & all) == all ? ~0ULL : (support & all)));
    replay(ops, SchedSink{sched});
    uint64_t sup = support & all;
    sched.finish([&](qsim::Pass &&ps) {
        if (cost_sweeps) *cost_sweeps += qsim::pass_time_cost(ps, false) / (32.0 * (double)(1ULL << m));
        if (ps.kclass != QSIM_K_TILE) { sup = all; return; } // a single-gate kernel: the engine writes the zeros out first
        sup |= qsim::tile_mask(ps.geom);
    });
    return sup & all;
}

// One placement policy with one hand-over limit, planned in full.  The circuit is consumed segment by segment: what can run
// where the qubits are now becomes a local step, the rest waits behind ONE exchange, and so on (build_plan_policy).
struct Planner {
    const int n, p, P, m;
    const bool full_swap; // an exchange swaps all p global qubits (choose_globals local_only)
    const int tail;       // largest last pass handed on across an exchange, in gate statements (tail_limit)
    // want_cost: also price the local steps (Plan::local_sweeps) — every holding shard's every segment is then scheduled even when
    // its support is already everything; without it only the segments whose support can still grow are (a few at the start of a run).
    const bool want_cost;
    Plan &plan;
    std::vector<int> pos; // logical -> physical
    uint64_t mixed = 0;   // logical qubits some gate may have moved away from |0> (a first, gate-level bound for Step::mixed_local)
    SupportWalk walk;     // ... and the bound the shards' engines will have themselves (scheduled_support), per shard

    Planner(int n_, int p_, Plan &plan_, bool full_swap_, int tail_, bool want_cost_)
        : n(n_), p(p_), P(1 << p_), m(n_ - p_), full_swap(full_swap_), tail(tail_), want_cost(want_cost_), plan(plan_), pos((size_t)n_), walk(n_ - p_, 0, 1 << p_) {
        plan.n = n; plan.p = p; plan.m = m;
        for (int q = 0; q < n; q++) pos[q] = q;
    }

    // With `ng` as the new global qubits: the ones among them that are local now, in ng's order, and the global ones that are
    // not among them, ascending.
    void leaving_and_entering(const std::vector<int> &ng, std::vector<int> &outgoing, std::vector<int> &incoming) const {
        for (int q : ng) if (pos[q] < m) outgoing.push_back(q);
        for (int q = 0; q < n; q++)
            if (pos[q] >= m && std::find(ng.begin(), ng.end(), q) == ng.end()) incoming.push_back(q);
    }

    void place_freely(const std::vector<LGate> &gates) { // |0...0> is the same under every placement: nothing moves
        std::vector<int> outgoing, incoming;
        leaving_and_entering(choose_globals(gates, pos, n, p, m), outgoing, incoming);
        for (size_t i = 0; i < outgoing.size() && i < incoming.size(); i++) std::swap(pos[outgoing[i]], pos[incoming[i]]);
    }

    // runnable: every qubit the gate needs local is, and no deferred gate in front of it shares a qubit with it
    void split(const std::vector<LGate> &remaining, std::vector<LGate> &run, std::vector<LGate> &deferred) const {
        uint64_t blocked = 0;
        for (const LGate &g : remaining) {
            uint64_t qs = 1ULL << g.q0;
            if (g.kind == QSIM_GATE_CX) qs |= 1ULL << g.q1;
            if (qs & blocked) { blocked |= qs; deferred.push_back(g); continue; }
            int q[2], c;
            needs_local(g, q, c);
            bool ok = true;
            for (int k = 0; k < c; k++) ok = ok && pos[q[k]] < m;
            if (ok) run.push_back(g);
            else { blocked |= qs; deferred.push_back(g); }
        }
    }

    // An exchange follows: a small last pass waits for it.
    // What the scheduler put into the last pass is only a PROPOSAL: it saw one shard's version of the segment (a CX controlled
    // by a shard-id bit as an X; on the shards where that bit is 0 there is no gate at all, and products that cancel on one
    // shard do not on another), so its order proves nothing for the others.  A gate may wait for the exchange if it
    // commutes, by what it IS — not by what some product of matrices happens to be —, with every gate of the segment
    // that comes after it in the circuit and stays: no shared qubit, or only qubits in which both are block-diagonal
    // (a diagonal gate, the control of a CX).  Gates that fail stay, which can make others fail: iterate.
    void hand_over_tail(std::vector<LGate> &run, std::vector<LGate> &deferred) {
        auto diag_mask = [](const LGate &g) -> uint64_t { // qubits the gate is block-diagonal in
            if (g.kind == QSIM_GATE_CX) return g.q0 == g.q1 ? 0 : 1ULL << g.q0;
            return g.diag() ? 1ULL << g.q0 : 0;
        };
        auto qubits = [](const LGate &g) -> uint64_t { return (1ULL << g.q0) | (g.kind == QSIM_GATE_CX ? 1ULL << g.q1 : 0); };
        std::vector<char> moving(run.size(), 0);
        for (size_t t : small_tail(run, pos, m, plan.steps.empty(), tail)) moving[t] = 1;
        for (bool changed = true; changed;) {
            changed = false;
            uint64_t later_mix = 0, later_any = 0; // over the staying gates behind the current position: qubits they mix / touch
            for (size_t i = run.size(); i-- > 0;) {
                const LGate &g = run[i];
                const uint64_t q = qubits(g), d = diag_mask(g);
                if (moving[i]) {
                    // shared qubits must be diagonal on both sides: none of g's qubits may be mixed later, none of g's mixed qubits touched later
                    if ((q & later_mix) || ((q & ~d) & later_any)) { moving[i] = 0; changed = true; }
                }
                if (!moving[i]) { later_mix |= q & ~d; later_any |= q; }
            }
        }
        std::vector<LGate> keep, moved;
        for (size_t i = 0; i < run.size(); i++) (moving[i] ? moved : keep).push_back(run[i]);
        if (moved.empty()) return;
        plan.tail_gates += (int)moved.size();
        moved.insert(moved.end(), deferred.begin(), deferred.end()); // in front of what was deferred already: nothing there precedes them on a shared qubit
        deferred.swap(moved);
        run.swap(keep);
    }

    // What `run` (in program order) is on shard r, in its local coordinates.
    std::vector<LocalOp> ops_on(int r, const std::vector<LGate> &run) const {
        std::vector<LocalOp> ops;
        for (const LGate &g : run) {
            LocalOp o{};
            if (g.kind == QSIM_GATE_CX) {
                if (g.q0 == g.q1) continue;
                if (pos[g.q0] < m) { o.kind = OpKind::cx; o.a = pos[g.q0]; o.b = pos[g.q1]; ops.push_back(o); }
                else if ((r >> (pos[g.q0] - m)) & 1) {
                    o.kind = OpKind::u1; o.a = pos[g.q1];
                    o.m[0] = 0; o.m[1] = 1; o.m[2] = 1; o.m[3] = 0;
                    ops.push_back(o);
                }
            } else if (pos[g.q0] < m) {
                o.kind = OpKind::u1; o.a = pos[g.q0];
                std::copy(g.m, g.m + 4, o.m);
                ops.push_back(o);
            } else {
                const int b = (r >> (pos[g.q0] - m)) & 1;
                const cd z = g.m[b ? 3 : 0];
                if (z != cd(1, 0)) { o.kind = OpKind::scale; o.m[0] = z; ops.push_back(o); }
            }
        }
        return ops;
    }

    void local_step(const std::vector<LGate> &run) {
        for (const LGate &g : run) { // in program order
            if (g.kind == QSIM_GATE_CX) { if (g.q0 != g.q1 && (mixed >> g.q0 & 1ULL)) mixed |= 1ULL << g.q1; }
            else if (!g.diag()) mixed |= 1ULL << g.q0;
        }
        if (run.empty()) return;
        Step st;
        for (int r = 0; r < P; r++) st.per_shard.push_back(ops_on(r, run));
        if (p) {
            double worst = 0; // the step takes as long as its busiest shard: the first and the last shard stand for all
            for (int r = 0; r < P; r++) {
                if (!walk.holds[(size_t)r]) continue;
                double cost = 0;
                const bool rep = want_cost && (r == 0 || r == P - 1);
                walk.sup[(size_t)r] = scheduled_support(st.per_shard[(size_t)r], m, walk.sup[(size_t)r], rep ? &cost : nullptr);
                worst = std::max(worst, cost);
            }
            plan.local_sweeps += worst;
        }
        plan.steps.push_back(std::move(st));
    }

    // The exchange that brings in what `deferred` needs next; false: no progress possible.
    bool exchange_step(const std::vector<LGate> &deferred) {
        std::vector<int> outgoing, incoming;
        leaving_and_entering(choose_globals(deferred, pos, n, p, m, full_swap), outgoing, incoming);
        std::sort(outgoing.begin(), outgoing.end(), [&](int a, int b) { return pos[a] < pos[b]; });
        std::sort(incoming.begin(), incoming.end(), [&](int a, int b) { return pos[a] < pos[b]; });
        const int k = (int)outgoing.size();
        if (k == 0 || k != (int)incoming.size()) return false;
        Step st;
        st.exchange = true;
        for (int q : outgoing) st.Lsel.push_back(pos[q]);
        for (int q : incoming) st.J.push_back(pos[q] - m);
        uint64_t gate_level = 0, engine_level = 0;
        for (int q = 0; q < n; q++)
            if ((mixed >> q & 1ULL) && pos[q] < m) gate_level |= 1ULL << pos[q];
        walk.held(engine_level, st.mixed_rank);
        st.mixed_local = gate_level & engine_level; // both are bounds on where the state can be non-zero
        walk.after_exchange(st);                    // what every shard holds afterwards
        std::vector<int> np(pos);
        for (int q = 0; q < n; q++)
            if (pos[q] < m && std::find(st.Lsel.begin(), st.Lsel.end(), pos[q]) == st.Lsel.end()) {
                int below = 0;
                for (int s : st.Lsel) below += s < pos[q];
                np[q] = pos[q] - below;
            }
        for (int i = 0; i < k; i++) np[incoming[i]] = m - k + i;
        for (int i = 0; i < k; i++) np[outgoing[i]] = m + st.J[i];
        pos = np;
        plan.steps.push_back(std::move(st));
        plan.exchanges++;
        return true;
    }
};

bool build_plan_policy(int n, int p, const std::vector<LGate> &gates, Plan &plan, bool full_swap, int tail, bool want_cost) {
    Planner pl(n, p, plan, full_swap, tail, want_cost);
    std::vector<LGate> remaining(gates);
    if (p && !remaining.empty()) pl.place_freely(remaining);
    while (!remaining.empty()) {
        std::vector<LGate> run, deferred;
        pl.split(remaining, run, deferred);
        if (p && !deferred.empty()) pl.hand_over_tail(run, deferred);
        pl.local_step(run);
        if (!deferred.empty() && !pl.exchange_step(deferred)) return false;
        remaining.swap(deferred);
    }
    plan.final_pos = pl.pos;
    return true;
}

// Exchange cost of a plan in integer units (so that the C++ planner and its Python twin decide identically): one
// exchange of k qubits = a pack pass over the shard (2 S bytes of HBM traffic) + 2^-k of the shard over each of 2^k - 1
// links in parallel.  With S / link = kLinkUnits and 2 S / HBM = kPackUnits (defaults: 50 GB/s per link direction, 5 TB/s
// pack kernel, i.e. 200 : 1 per byte; qsim_shard_plan_predict takes the real figures) the cost is additive.
constexpr long kLinkUnits = 25600, kPackUnits = 256;
long plan_cost(const Plan &plan) {
    long c = 0;
    for (const Step &st : plan.steps)
        if (st.exchange) c += kPackUnits + (kLinkUnits >> st.J.size());
    return c;
}

// One sweep of a shard in plan_cost's units: 2 S bytes at the tile kernel's ~4.5 TB/s against S over a 50 GB/s link = kLinkUnits.
constexpr double kSweepUnits = 570.0;

} // namespace

// The placement policies (keep far-next-use globals / swap all log2 P of them) and, unless QSIM_SHARD_TAIL pins it, a few
// limits for the hand-over of a segment's small last pass are planned in full; the plan with the least predicted time — the
// exchanges over the links (plan_cost) plus the local steps on their busiest shard (Plan::local_sweeps: the segments scheduled
// with the engine's own scheduler and priced by pass_time_cost) — is kept; ties keep the first.  With QSIM_SHARD_TAIL set only
// the two policies are compared, by their exchanges alone: the planner proper, which tests/py_shard_plan.py restates.
bool build_plan(int n, int p, const std::vector<LGate> &gates, Plan &plan) {
    const bool pinned = getenv("QSIM_SHARD_TAIL") != nullptr;
    // the search schedules every segment of every candidate plan: seconds for the circuits it is meant for (thousands of
    // gates on registers that need many GPUs), minutes for a 400 000-gate file like the reference's own benchmark circuits
    // (OverallTest.csv) — those get the default plan
    const bool search = !pinned && p > 0 && gates.size() <= 20000;
    std::vector<int> tails{tail_limit()};
    if (search) for (int t : {0, 12, 40}) tails.push_back(t);
    bool have = false;
    double best = 0;
    for (int tail : tails)
        for (int full = 0; full < (p > 1 ? 2 : 1); full++) {
            Plan cand;
            if (!build_plan_policy(n, p, gates, cand, full != 0, tail, search)) { if (!have && tail == tails[0] && full == 0) return false; continue; }
            const double cost = (double)plan_cost(cand) + (search ? kSweepUnits * cand.local_sweeps : 0.0);
            if (!have || cost < best) { best = cost; plan = std::move(cand); have = true; }
        }
    return have;
}

} // namespace shard

using namespace shard;

// ---- the plan as an object (host only): what distributed.py's one-process-per-GPU driver executes -------------
extern "C" int qsim_shard_plan_create(qsim_shard_plan **out, const qsim_circuit *circ, int num_shards) {
    if (!out || !circ) return cfail(QSIM_ERR_ARG, "NULL argument");
    *out = nullptr;
    int p = 0;
    if (int rc = check_shards(circ->num_q, num_shards, &p)) return rc;
    if (int rc = check_shardable(circ, -1, "shards")) return rc;
    std::vector<LGate> gates;
    gates_of(circ, gates);
    qsim_shard_plan *sp = new qsim_shard_plan();
    sp->P = num_shards;
    if (!build_plan(circ->num_q, p, gates, sp->plan)) {
        delete sp;
        return cfail(QSIM_ERR_ARG, "planner made no progress");
    }
    *out = sp;
    return QSIM_OK;
}

extern "C" void qsim_shard_plan_free(qsim_shard_plan *p) { delete p; }
extern "C" int qsim_shard_plan_num_steps(const qsim_shard_plan *p) { return p ? (int)p->plan.steps.size() : -1; }

extern "C" int qsim_shard_plan_step(const qsim_shard_plan *p, int step, int *kind, int *k, int *shard_bits, int *local_bits) {
    if (!p || step < 0 || step >= (int)p->plan.steps.size()) return QSIM_ERR_ARG;
    const Step &st = p->plan.steps[step];
    if (kind) *kind = st.exchange ? 1 : 0;
    if (k) *k = (int)st.J.size();
    for (size_t i = 0; i < st.J.size(); i++) {
        if (shard_bits) shard_bits[i] = st.J[i];
        if (local_bits) local_bits[i] = st.Lsel[i];
    }
    return QSIM_OK;
}

extern "C" int qsim_shard_plan_step_support(const qsim_shard_plan *p, int step, uint64_t *mixed_local, uint64_t *mixed_rank) {
    if (!p || step < 0 || step >= (int)p->plan.steps.size() || !p->plan.steps[(size_t)step].exchange) return QSIM_ERR_ARG;
    if (mixed_local) *mixed_local = p->plan.steps[(size_t)step].mixed_local;
    if (mixed_rank) *mixed_rank = p->plan.steps[(size_t)step].mixed_rank;
    return QSIM_OK;
}

extern "C" int qsim_shard_plan_exchange_roles(const qsim_shard_plan *p, int step, int shard, qsim_exchange_roles *out) {
    if (!p || !out || step < 0 || step >= (int)p->plan.steps.size() || shard < 0 || shard >= p->P || !p->plan.steps[(size_t)step].exchange) return QSIM_ERR_ARG;
    const Roles r = roles_of(shard, p->plan.m, p->plan.steps[(size_t)step]);
    out->mine = r.mine; out->empty_before = r.empty_before; out->empty_after = r.empty_after; out->keep_own = r.keep_own;
    out->send = r.send; out->recv = r.recv; out->unread = r.unread; out->new_support = r.new_support;
    return QSIM_OK;
}

extern "C" int qsim_shard_plan_final_pos(const qsim_shard_plan *p, int *pos) {
    if (!p || !pos) return QSIM_ERR_ARG;
    for (size_t q = 0; q < p->plan.final_pos.size(); q++) pos[q] = p->plan.final_pos[q];
    return QSIM_OK;
}

namespace {
// The ops as include/qsim.h documents them for the callback: the kind as its integer, what an op does not use as zeros.
struct CallbackSink {
    qsim_local_op_cb cb;
    void *user;
    int cx(int a, int b) { const double none[8] = {}; cb(user, (int)OpKind::cx, a, b, none); return 0; }
    int u1(const cd *m, int a) { cb(user, (int)OpKind::u1, a, 0, as_doubles(m)); return 0; }
    int scale(cd z) { const double m[8] = {z.real(), z.imag()}; cb(user, (int)OpKind::scale, 0, 0, m); return 0; }
};
} // namespace

extern "C" int qsim_shard_plan_local_ops(const qsim_shard_plan *p, int step, int shard, qsim_local_op_cb cb, void *user) {
    if (!p || !cb || step < 0 || step >= (int)p->plan.steps.size() || shard < 0 || shard >= p->P) return QSIM_ERR_ARG;
    const Step &st = p->plan.steps[step];
    if (st.exchange) return QSIM_ERR_ARG;
    return replay(st.per_shard[shard], CallbackSink{cb, user});
}

// Predicted exchange cost of the plan on one fully connected xGMI node: bytes each rank sends, and the time of the
// exchanges alone (pack pass + the largest per-link transfer; a k-qubit swap puts 2^-k of the shard on each of 2^k - 1
// links, both directions at once).  link_gbps is per link and direction, pack_gbps the pack kernel's HBM rate.
extern "C" int qsim_shard_plan_predict(const qsim_shard_plan *p, double link_gbps, double pack_gbps, double *bytes_per_rank, double *seconds) {
    if (!p || link_gbps <= 0 || pack_gbps <= 0) return QSIM_ERR_ARG;
    const double S = 16.0 * (double)(1ULL << p->plan.m);
    double bytes = 0, secs = 0;
    for (const Step &st : p->plan.steps) {
        if (!st.exchange) continue;
        const int k = (int)st.J.size();
        const double blk = S / (double)(1 << k);
        bytes += blk * ((1 << k) - 1);
        secs += 2.0 * S / (pack_gbps * 1e9) + blk / (link_gbps * 1e9);
    }
    if (bytes_per_rank) *bytes_per_rank = bytes;
    if (seconds) *seconds = secs;
    return QSIM_OK;
}
