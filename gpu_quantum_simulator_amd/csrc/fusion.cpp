// fusion.cpp — the scheduler's first half (scheduler.h): FusedOp predicates, the fusion algebra, the cluster state machine that folds
// the gate stream into closed clusters, and the configuration (the QSIM_SCHED_* knob table, engine_sched_config).  Pure host code;
// exercised on the CPU by tests/test_scheduler_cpu.py through qsim_schedule_circuit().
#include "scheduler_impl.h"

#include <cstdlib>

namespace qsim {

using sched::is_one;
using sched::is_zero;
using sched::make_op;

static const cd kI2[4] = {cd(1, 0), cd(0, 0), cd(0, 0), cd(1, 0)};

bool FusedOp::is_diag() const {
    if (kind == OP_CX) return false;
    const int d = dim();
    for (int r = 0; r < d; r++)
        for (int c = 0; c < d; c++)
            if (r != c && !is_zero(m[d * r + c])) return false;
    return true;
}

uint64_t FusedOp::selector_mask() const {
    if (kind == OP_CX) return 1ULL << q_hi; // the control
    const int k = nq(), d = dim();
    const int qs[2] = {q_hi, q_lo};
    uint64_t out = 0;
    for (int a = 0; a < k; a++) {
        const int bit = 1 << (k - 1 - a); // position of qs[a] in the row/column index
        bool ok = true;
        for (int r = 0; r < d && ok; r++)
            for (int c = 0; c < d; c++)
                if (((r ^ c) & bit) && !is_zero(m[d * r + c])) { ok = false; break; }
        if (ok) out |= 1ULL << qs[a];
    }
    return out;
}

// EXACT identity only: the reference's isIdentity tolerance of 1e-3 (quantum_simulator_4x4.cu:247-250)
// silently drops and reorders small rotations.
bool FusedOp::is_identity() const {
    if (!is_diag()) return false;
    const int d = dim();
    for (int r = 0; r < d; r++)
        if (!is_one(m[(d + 1) * r])) return false;
    return true;
}

// ---- fusion algebra (own formulation of quantum_simulator_4x4.cu:148-233) -----------------------------
void Scheduler::mul2(const cd a[4], const cd b[4], cd out[4]) {
    cd t[4];
    for (int r = 0; r < 2; r++)
        for (int c = 0; c < 2; c++) t[2 * r + c] = a[2 * r] * b[c] + a[2 * r + 1] * b[2 + c];
    std::copy(t, t + 4, out);
}

void Scheduler::mul4(const cd a[16], const cd b[16], cd out[16]) {
    cd t[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            cd s(0, 0);
            for (int k = 0; k < 4; k++) s += a[4 * r + k] * b[4 * k + c];
            t[4 * r + c] = s;
        }
    std::copy(t, t + 16, out);
}

// (hi (x) lo)[(i1 i2), (j1 j2)] = hi[i1][j1] * lo[i2][j2]
void Scheduler::kron(const cd hi[4], const cd lo[4], cd out[16]) {
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) out[4 * r + c] = hi[2 * (r >> 1) + (c >> 1)] * lo[2 * (r & 1) + (c & 1)];
}

// CX as a permutation of the basis |hi lo>: control on the high bit exchanges |10> and |11>, control on
// the low bit exchanges |01> and |11>.
void Scheduler::cx4(bool control_is_hi, cd out[16]) {
    const int perm_hi[4] = {0, 1, 3, 2}, perm_lo[4] = {0, 3, 2, 1};
    const int *p = control_is_hi ? perm_hi : perm_lo;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) out[4 * r + c] = cd(p[r] == c ? 1.0 : 0.0, 0.0);
}

// std::complex multiplication may go through the Annex-G slow path; these matrices are tiny and only
// built on the host, so that is irrelevant.  Zeros stay exact: every term of an off-diagonal entry of a
// product of diagonal matrices has an exact-zero factor.

// The QSIM_SCHED_* variables override the search parameters for experiments (tools/); they are not
// part of the API and change the pass count, never the result (scheduler.h SchedEnv).  One entry per variable, in the order of
// the bits of SchedEnv::set: the name, where its value is kept (an int read with atoi, a double read with atof, or nowhere: the
// variable counts by being present) and what it does to a configuration.  read_sched_env, apply_sched_env and the equality of two
// records go over this table and nothing else, so a variable cannot be read without being applied and compared.
namespace {
struct Knob {
    const char *name;
    int SchedEnv::*ival;
    double SchedEnv::*dval;
    void (*apply)(const SchedEnv &e, SchedConfig &cfg);
};
const Knob kKnobs[] = {
    {"QSIM_SCHED_LOOKAHEAD", &SchedEnv::lookahead, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.lookahead = e.lookahead; }},
    {"QSIM_SCHED_ROLLOUT", &SchedEnv::rollout, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.rollout = e.rollout; }},
    {"QSIM_SCHED_WINDOW", &SchedEnv::window, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.window = e.window; }},
    {"QSIM_SCHED_LOCAL", &SchedEnv::local_iters, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.local_iters = e.local_iters; }},
    {"QSIM_SCHED_OBJ", &SchedEnv::objective, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.objective = e.objective; }},
    {"QSIM_SCHED_MERGE", &SchedEnv::merge, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.merge = e.merge; }},
    {"QSIM_SCHED_MERGEQ", &SchedEnv::merge_qubits, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.merge_qubits = e.merge_qubits; }},
    {"QSIM_SCHED_CAP", &SchedEnv::cap, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.tile_max_ops = e.cap; c.tail_max_ops = 0; }},
    {"QSIM_SCHED_CHEAP", nullptr, &SchedEnv::cheap_margin, [](const SchedEnv &e, SchedConfig &c) { c.cheap_margin = e.cheap_margin; }},
    {"QSIM_SCHED_NOCOMMUTE", nullptr, nullptr, [](const SchedEnv &, SchedConfig &c) { c.commute = 0; }},
    {"QSIM_SCHED_SEED", &SchedEnv::seed, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.seed = (uint64_t)e.seed; }},
    {"QSIM_SCHED_SUPW", &SchedEnv::support_weight, nullptr, [](const SchedEnv &e, SchedConfig &c) { c.support_weight = e.support_weight; }},
};
constexpr int kNumKnobs = (int)(sizeof kKnobs / sizeof kKnobs[0]);
} // namespace

SchedEnv read_sched_env() {
    SchedEnv e;
    for (int bit = 0; bit < kNumKnobs; bit++) {
        const Knob &k = kKnobs[bit];
        const char *v = getenv(k.name);
        if (!v) continue;
        if (k.ival) e.*k.ival = atoi(v);
        if (k.dval) e.*k.dval = atof(v);
        e.set |= 1u << bit;
    }
    return e;
}

void apply_sched_env(const SchedEnv &e, SchedConfig &cfg) {
    for (int bit = 0; bit < kNumKnobs; bit++)
        if ((e.set >> bit) & 1u) kKnobs[bit].apply(e, cfg);
}

bool SchedEnv::operator==(const SchedEnv &o) const {
    if (set != o.set) return false;
    for (const Knob &k : kKnobs) {
        if (k.ival && this->*k.ival != o.*k.ival) return false;
        if (k.dval && this->*k.dval != o.*k.dval) return false;
    }
    return true;
}

static SchedConfig with_env(SchedConfig cfg) { apply_sched_env(read_sched_env(), cfg); return cfg; }

Scheduler::Scheduler(const SchedConfig &cfg) : cfg_(with_env(cfg)), tile_(cfg_), open_(cfg.n > 0 ? cfg.n : 0, -1) {
    if (cfg_.affine_support && cfg_.fuse >= 3) tracker_.start(cfg_.n, cfg_.initial_support);
}

SchedConfig engine_sched_config(int n, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops, int pad_from, bool f32, uint64_t initial_support) {
    SchedConfig c;
    c.pad_from = pad_from;
    c.initial_support = initial_support; // 0: the run starts from a reset (what the planning entry points assume)
    c.n = n; c.fuse = fuse; c.tile_bits = tile_bits; c.tile_low_bits = tile_low_bits; c.tile_max_ops = tile_max_ops;
    // The pass-set local search (SchedConfig::local_iters with one pass of lookahead) cost ~1.5 ms of host time per pass when the
    // thresholds below were measured (~0.7 ms since the scans of build_passes became incremental).  Passes are launched as they are produced, so the search is free once a pass runs longer than that on the
    // GPU: from 4 GiB of state (n = 28 fp64: 1.9 ms per pass).  Since the row-class form of the sparse blocks (one LDS
    // read per amplitude) most passes are bound by their memory time again, so one pass less is ~7 ms less at n = 30
    // (round 1: the fuller passes were LDS-bound and the total did not move).  With the search on, a pass is capped at
    // 24 clusters (5-6 merged blocks): ~1.6 + 0.8 ms per block then stays under the pass's ~6.8 ms of memory time.
    // Twelve seeded 1000-gate circuits at n = 30: 204 passes without the search, 188 with it (191 / 193 with two /
    // three passes of lookahead, which also cost more host time, so one it is).  n = 30 bench circuit: 16 passes /
    // 119.7 ms without, 15 / 115.5 ms with; n = 28: 31.1 -> 29.8 ms; n = 32: 471 -> 451 ms; n = 26 would LOSE (8.5 -> 9.9 ms,
    // the host becomes the bottleneck), hence the threshold.  QSIM_SCHED_LOCAL / QSIM_SCHED_LOOKAHEAD override.
    const int size_class = n - (f32 ? 1 : 0); // log2 of the state size in 16-byte units
    if (fuse >= 3 && size_class >= 28) {
        c.local_iters = 3;
        c.lookahead = 1;
        // Round 3 re-measured the cap with the cheaper block phase of round 2 (tools/cap_sweep.py, five seeded circuits at n = 30, no
        // planning step): 24 clusters 404 ms in total, 28 373 ms, 32 385 ms, 40 374 ms — and no single value is best for every
        // circuit (per-circuit minima add up to 363 ms), so 28 is the default and the planning step tries 24 / 32 / 40 as well.
        if (tile_max_ops == 32) { c.tile_max_ops = 28; c.tail_max_ops = 32; } // 32 = the option's default, i.e. not chosen by the caller
    }
    return c;
}

// ---- clusters: the ONE way each comes to be ------------------------------------------------------------------------------
FusedOp sched::make_op(int kind, int q_hi, int q_lo, const cd *m, uint32_t gates) {
    FusedOp op;
    op.kind = kind; op.q_hi = q_hi; op.q_lo = q_lo; op.gates = gates;
    if (m) std::copy(m, m + op.dim() * op.dim(), op.m);
    return op;
}

void Scheduler::open_cluster(const FusedOp &op, std::vector<uint32_t> src) {
    pool_.push_back(op);
    if (cfg_.track) pool_src_.push_back(std::move(src));
    open_[op.q_hi] = (int)pool_.size() - 1;
    if (op.kind == OP_G2) open_[op.q_lo] = (int)pool_.size() - 1;
}

void Scheduler::append_closed(const FusedOp &op, uint32_t g) {
    closed_.push_back(op);
    if (cfg_.track) closed_src_.push_back({g});
}

void Scheduler::close(int idx) {
    if (idx < 0) return;
    FusedOp &op = pool_[idx];
    open_[op.q_hi] = -1;
    if (op.kind == OP_G2) open_[op.q_lo] = -1;
    if (!op.is_identity()) {
        closed_.push_back(op);
        if (cfg_.track) closed_src_.push_back(std::move(pool_src_[(size_t)idx]));
    }
    op.kind = 0;
}

// SchedConfig::defer_flips: out = X^f U X^f for the flips `fm` on the gate's qubits, as a bit mask of its row index.  Entries are
// moved, never multiplied: exact zeros and the diagonal stay what they are (selector_mask and the merge conditions read them).
static void conjugate_by_flips(const cd *U, int dim, int fm, cd *out) {
    for (int r = 0; r < dim; r++)
        for (int c = 0; c < dim; c++) out[dim * r + c] = U[dim * (r ^ fm) + (c ^ fm)];
}

void Scheduler::add_1q(const cd Uin[4], int q) {
    const cd *U = Uin;
    cd conj[4], diag[4];
    if (deferring()) {
        if (flips_ >> q & 1ULL) { conjugate_by_flips(Uin, 2, 1, conj); U = conj; }
        if (is_zero(U[0]) && is_zero(U[3])) { // anti-diagonal: A = X (X A), and X A = diag(A[1][0], A[0][1]) — the X is owed from here on
            flips_ ^= 1ULL << q;
            if (is_one(U[1]) && is_one(U[2])) { deferred_.push_back((uint32_t)gates_++); return; } // X itself: nothing is left to schedule
            diag[0] = U[2]; diag[1] = diag[2] = cd(0, 0); diag[3] = U[1];
            U = diag;
        }
    }
    const uint32_t g = (uint32_t)gates_++;
    const FusedOp op = make_op(OP_G1, q, -1, U);
    if (cfg_.fuse == 0) { append_closed(op, g); return; }
    const int idx = open_[q];
    if (idx < 0) { open_cluster(op, {g}); return; }
    // Level 3 keeps a pair cluster block-diagonal in a qubit for as long as it can: such a cluster can run in passes
    // whose tile does not contain that qubit.  A gate that would mix the qubit's halves starts a new cluster instead
    // (inside one pass the two are merged again by merge_blocks).
    if (cfg_.fuse >= 3 && cfg_.selectors && pool_[idx].kind == OP_G2 && (!is_zero(U[1]) || !is_zero(U[2])) &&
        (pool_[idx].selector_mask() >> q & 1ULL)) {
        close(idx);
        open_cluster(op, {g});
        return;
    }
    FusedOp &c = pool_[idx];
    c.gates++;
    if (cfg_.track) pool_src_[(size_t)idx].push_back(g);
    if (c.kind == OP_G1) {
        mul2(U, c.m, c.m); // later gate multiplies from the left
    } else {
        cd e[16];
        if (q == c.q_hi) kron(U, kI2, e);
        else kron(kI2, U, e);
        mul4(e, c.m, c.m);
    }
}

void Scheduler::add_cx(int control, int target) {
    const uint32_t g = (uint32_t)gates_++;
    if (control == target) return; // quantum_simulator.c:99: a silent no-op
    if (cfg_.fuse <= 1) {
        if (cfg_.fuse == 1) { close(open_[control]); close(open_[target]); }
        append_closed(make_op(OP_CX, control, target, nullptr), g);
        return;
    }
    cd m[16];
    cx4(control > target, m);
    const int q_hi = std::max(control, target), q_lo = std::min(control, target);
    if (const int fm = deferring() ? flips_on(q_hi, q_lo) : 0) { // a flipped target changes nothing, a flipped control gives "control = 0"
        cd conj[16];
        conjugate_by_flips(m, 4, fm, conj);
        std::copy(conj, conj + 16, m);
    }
    fold_2q(m, q_hi, q_lo, 1, g);
}

void Scheduler::add_2q(const cd U[16], int q_hi, int q_lo) {
    const uint32_t g = (uint32_t)gates_++;
    if (cfg_.fuse <= 1) {
        if (cfg_.fuse == 1) { close(open_[q_hi]); close(open_[q_lo]); }
        append_closed(make_op(OP_G2, q_hi, q_lo, U), g);
        return;
    }
    cd conj[16];
    if (const int fm = deferring() ? flips_on(q_hi, q_lo) : 0) { conjugate_by_flips(U, 4, fm, conj); U = conj; }
    fold_2q(U, q_hi, q_lo, 1, g);
}

void Scheduler::fold_2q(const cd U[16], int q_hi, int q_lo, uint32_t gates, uint32_t g) {
    int ia = open_[q_hi], ib = open_[q_lo];
    if (ia >= 0 && ia == ib) { // the pair is already one cluster: keep folding
        FusedOp &c = pool_[ia];
        mul4(U, c.m, c.m);
        c.gates += gates;
        if (cfg_.track) pool_src_[(size_t)ia].push_back(g);
        return;
    }
    // a cluster shared with a third qubit has to run first
    if (ia >= 0 && pool_[ia].kind == OP_G2) { close(ia); ia = -1; }
    if (ib >= 0 && pool_[ib].kind == OP_G2) { close(ib); ib = -1; }
    if (cfg_.fuse >= 3 && cfg_.selectors) {
        // same idea when the pair cluster is created: a pending 1-qubit product that is not diagonal would destroy
        // the block-diagonal structure U has in that qubit (e.g. the control of a CX) — let it run on its own
        const uint64_t sel = make_op(OP_G2, q_hi, q_lo, U).selector_mask();
        if (ia >= 0 && (sel >> q_hi & 1ULL) && !pool_[ia].is_diag()) { close(ia); ia = -1; }
        if (ib >= 0 && (sel >> q_lo & 1ULL) && !pool_[ib].is_diag()) { close(ib); ib = -1; }
    }
    FusedOp op = make_op(OP_G2, q_hi, q_lo, nullptr, gates);
    const cd *a = kI2, *b = kI2;
    if (ia >= 0) { a = pool_[ia].m; op.gates += pool_[ia].gates; }
    if (ib >= 0) { b = pool_[ib].m; op.gates += pool_[ib].gates; }
    cd k[16];
    kron(a, b, k);
    mul4(U, k, op.m);
    if (ia >= 0) pool_[ia].kind = 0;
    if (ib >= 0) pool_[ib].kind = 0;
    std::vector<uint32_t> src;
    if (cfg_.track) {
        if (ia >= 0) src = std::move(pool_src_[(size_t)ia]);
        if (ib >= 0) src.insert(src.end(), pool_src_[(size_t)ib].begin(), pool_src_[(size_t)ib].end());
        src.push_back(g);
    }
    open_cluster(op, std::move(src));
}

void Scheduler::finish(const PassSink &out) {
    const PassSink sink = [&](Pass &&p) { tracker_.visit(p); out(std::move(p)); }; // every pass, in the order it will run
    for (int q = 0; q < cfg_.n; q++) close(open_[q]);
    pool_.clear();
    pool_src_.clear();
    if (deferred_.empty()) build_passes(sink);
    else { // the deferred X statements count with the last pass, so that one is held back until the end is seen
        Pass last;
        bool have = false;
        build_passes([&](Pass &&p) {
            if (have) sink(std::move(last));
            last = std::move(p);
            have = true;
        });
        if (have) {
            (last.blocks.empty() ? last.ops.back().gates : last.blocks.back().gates) += (uint32_t)deferred_.size();
            if (cfg_.track) last.src.insert(last.src.end(), deferred_.begin(), deferred_.end());
            sink(std::move(last));
        }
        deferred_.clear();
    }
    closed_.clear();
    closed_src_.clear();
}

void Scheduler::finish(std::vector<Pass> &out) {
    finish([&out](Pass &&p) { out.push_back(std::move(p)); });
}

} // namespace qsim
