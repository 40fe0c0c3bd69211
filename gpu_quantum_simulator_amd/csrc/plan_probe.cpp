// plan_probe.cpp — the calls that say how a circuit WOULD be scheduled without running anything: qsim_plan_circuit*, qsim_plan_passes,
// qsim_schedule_circuit*, qsim_tile_records.  They take a circuit and the options that shape a schedule, never a qsim_state, and make
// no HIP call: the CPU tests and tools/sched_digest.py stand on them.  Also queue_of and schedule, which planning.cpp shares (planning.h).
#include <chrono>
#include <cstring>

#include "planning.h"

using namespace qsim;

std::vector<QueuedGate> qsim::queue_of(const qsim_circuit *c) {
    std::vector<QueuedGate> q;
    q.reserve((size_t)c->count);
    for (long i = 0; i < c->count; i++) q.emplace_back(*c, c->gates[i]);
    return q;
}

std::vector<Pass> qsim::schedule(const SchedConfig &cfg, const std::vector<QueuedGate> &gates, uint64_t *gates_seen, uint64_t *residual_flips) {
    Scheduler sv(cfg);
    feed(sv, gates);
    std::vector<Pass> passes;
    sv.finish(passes);
    if (gates_seen) *gates_seen = sv.gates_seen();
    if (residual_flips) *residual_flips = sv.residual_flips();
    return passes;
}

namespace {
// What a probe is asked about, beside the circuit and the fuse level: the options of a state that shape its schedules.
struct ProbeShape {
    int tile_bits, tile_low_bits, tile_max_ops = 32;
    uint64_t initial_support = 0;
    bool defer = false; // the X gates left to an index flip (SchedConfig::defer_flips): residual_flips says which
    bool affine = false; // the passes carry their PassRegion (SchedConfig::affine_support)
    const qsim_sched_setting *setting = nullptr; // the scheduler setting of a planning candidate on top (its defer counts, not `defer`)
};

SchedHint hint_of(const qsim_sched_setting &h, const SchedConfig &own) { // fields left open take the configuration's own value
    return {h.commute < 0 ? own.commute : h.commute, h.cheap_margin > 0 ? h.cheap_margin : own.cheap_margin, h.lookahead < 0 ? own.lookahead : h.lookahead,
            h.cap, h.seed, h.defer != 0 ? 1 : 0, h.support_weight};
}
qsim_sched_setting setting_of(const SchedHint &h, double cost, bool is_default) {
    qsim_sched_setting o{};
    o.commute = h.commute; o.lookahead = h.lookahead; o.cap = h.cap; o.defer = h.defer; o.support_weight = h.support_weight;
    o.is_default = is_default ? 1 : 0; o.seed = h.seed; o.cheap_margin = h.cheap_margin; o.cost_bytes = cost;
    return o;
}

// How every probe opens: the arguments checked (have_args: the caller's pointers are all there) and the circuit scheduled as an
// fp64 state with these options would schedule it.
int probe_passes(bool have_args, const qsim_circuit *c, int fuse, const ProbeShape &shape, std::vector<Pass> &passes, uint64_t *gates_seen = nullptr,
                 uint64_t *residual_flips = nullptr) {
    if (!have_args || !c) return fail(QSIM_ERR_ARG, "NULL argument");
    if (fuse < 0 || fuse > 3) return fail(QSIM_ERR_ARG, "fuse level %d not in 0..3", fuse);
    SchedConfig cfg = engine_sched_config(c->num_q, fuse, shape.tile_bits, shape.tile_low_bits, shape.tile_max_ops, 10, false, shape.initial_support);
    cfg.defer_flips = shape.defer ? 1 : 0;
    cfg.affine_support = shape.affine ? 1 : 0;
    if (shape.setting) {
        if (shape.setting->cap < 0 || shape.setting->cap > 512 || shape.setting->support_weight < 0) return fail(QSIM_ERR_ARG, "scheduler setting out of range");
        cfg = with_hint(cfg, hint_of(*shape.setting, cfg));
    }
    passes = schedule(cfg, queue_of(c), gates_seen, residual_flips);
    return QSIM_OK;
}

// A block as the probes report it: ONE matrix, as (re, im) doubles, on (selecting qubits..., tile qubits...).
struct BlockView {
    std::vector<cd> full = std::vector<cd>((size_t)256 * 256);
    std::vector<double> matrix = std::vector<double>((size_t)2 * 256 * 256);
    int qubits[kMaxBlockQ + 2], nq = 0;
    void set(const TileBlock &blk) {
        nq = 0;
        for (int a = 0; a < blk.ns; a++) qubits[nq++] = blk.s[a];
        for (int a = 0; a < blk.nq; a++) qubits[nq++] = blk.q[a];
        const int D = 1 << nq;
        blk.full_matrix(full.data());
        for (int k = 0; k < D * D; k++) { matrix[2 * k] = full[k].real(); matrix[2 * k + 1] = full[k].imag(); }
    }
};

int report_schedule(const std::vector<Pass> &passes, qsim_sched_cb cb, void *user) {
    int pi = 0;
    BlockView view;
    for (const Pass &p : passes) {
        for (const FusedOp &op : p.ops) {
            double U[128];
            const int d = op.kind == OP_CX ? 0 : op.dim();
            for (int k = 0; k < d * d; k++) { U[2 * k] = op.m[k].real(); U[2 * k + 1] = op.m[k].imag(); }
            const int kind = op.kind == OP_G1 ? QSIM_GATE_U1 : op.kind == OP_CX ? QSIM_GATE_CX : QSIM_GATE_U2;
            const int qs[2] = {op.q_hi, op.q_lo};
            cb(user, pi, p.kclass, kind, qs, op.kind == OP_CX ? 2 : op.nq(), d ? U : nullptr, (int)op.gates);
        }
        for (const TileBlock &blk : p.blocks) {
            TileOp t;
            if (!to_tile_op(p.geom, blk, t)) return fail(QSIM_ERR_ARG, "internal: block does not fit its tile pass");
            view.set(blk);
            static const int kinds[9] = {0, QSIM_GATE_U1, QSIM_GATE_U2, QSIM_GATE_U3, QSIM_GATE_U4, QSIM_GATE_U5, QSIM_GATE_U6, QSIM_GATE_U7, QSIM_GATE_U8};
            cb(user, pi, p.kclass, kinds[view.nq], view.qubits, view.nq, view.matrix.data(), (int)blk.gates);
        }
        pi++;
    }
    return QSIM_OK;
}
} // namespace

static void fill_regions(const qsim_circuit *c, const std::vector<Pass> &passes, qsim_pass_region *out, int cap);

extern "C" int qsim_plan_circuit(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, qsim_stats *out) {
    return qsim_plan_circuit_from(c, fuse, tile_bits, tile_low_bits, 0, out);
}

extern "C" int qsim_plan_circuit_from(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, uint64_t initial_support, qsim_stats *out) {
    std::vector<Pass> passes;
    uint64_t gates = 0;
    QSIM_TRY(probe_passes(out != nullptr, c, fuse, {tile_bits, tile_low_bits, 32, initial_support}, passes, &gates));
    memset(out, 0, sizeof *out);
    out->gates = gates;
    for (const Pass &p : passes) { // a run from a reset: the first tile passes visit part of the register (Pass::visited)
        out->launches++;
        out->algorithmic_bytes += p.moved();
        out->k_launches[p.kclass]++;
        out->k_bytes[p.kclass] += p.moved();
    }
    return QSIM_OK;
}

// The same schedule pass by pass: which qubits each tile pass holds in its tile, how much of the register it visits and what the
// planning steps price it at.  What a host-side model needs to decide which passes could run chunk by chunk beside an exchange
// (bench.py exchange_model: a pass can only be pipelined over index bits that are NOT in its tile).
extern "C" int qsim_plan_passes(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, uint64_t initial_support, qsim_pass_info *out, int cap,
                                int *count) {
    std::vector<Pass> passes;
    QSIM_TRY(probe_passes(count && !(cap > 0 && !out), c, fuse, {tile_bits, tile_low_bits, 32, initial_support}, passes));
    *count = (int)passes.size();
    for (size_t i = 0; i < passes.size() && (int)i < cap; i++) {
        const Pass &p = passes[i];
        qsim_pass_info &o = out[i];
        o.kernel_class = p.kclass;
        o.blocks = p.kclass == QSIM_K_TILE ? (int)p.blocks.size() - p.geom.n_scale : 1;
        o.tile_mask = p.kclass == QSIM_K_TILE ? tile_mask(p.geom) : index_mask(c->num_q); // a single-gate kernel: treat every bit as touched
        o.visited = p.visited;
        o.bytes = p.moved();
        o.cost_bytes = pass_time_cost(p, false);
    }
    return QSIM_OK;
}

extern "C" int qsim_plan_regions(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support, int defer,
                                 qsim_pass_region *out, int cap, int *count) {
    std::vector<Pass> passes;
    QSIM_TRY(probe_passes(count && !(cap > 0 && !out), c, fuse, {tile_bits, tile_low_bits, tile_max_ops, initial_support, defer != 0, true}, passes));
    *count = (int)passes.size();
    fill_regions(c, passes, out, cap);
    return QSIM_OK;
}

static void fill_regions(const qsim_circuit *c, const std::vector<Pass> &passes, qsim_pass_region *out, int cap) {
    for (size_t i = 0; i < passes.size() && (int)i < cap; i++) {
        const Pass &p = passes[i];
        const PassRegion &r = p.region;
        qsim_pass_region &o = out[i];
        memset(&o, 0, sizeof o);
        o.kernel_class = p.kclass;
        o.tile_mask = p.kclass == QSIM_K_TILE ? tile_mask(p.geom) : index_mask(c->num_q);
        o.on = r.on ? 1 : 0;
        o.refined = r.refined ? 1 : 0;
        o.support_before = r.support_before;
        o.origin = r.origin;
        o.n_gen = (int)r.gen.size();
        for (size_t j = 0; j < r.gen.size() && j < 64; j++) o.gen[j] = r.gen[j];
        o.n_checks = (int)r.checks.size();
        for (size_t j = 0; j < r.checks.size() && j < 64; j++) { o.check_mask[j] = r.checks[j].mask; o.check_parity |= (uint64_t)(r.checks[j].parity & 1) << j; }
        o.visited = r.on ? r.visited : p.visited;
        o.read_share = r.on ? r.read_share : p.read_share;
    }
}

// The probes of one candidate of the planning step: the blocks and the regions of the schedule under that setting (level 3).
extern "C" int qsim_schedule_circuit_with(const qsim_circuit *c, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support,
                                          const qsim_sched_setting *setting, qsim_sched_cb cb, void *user, uint64_t *flip_mask) {
    std::vector<Pass> passes;
    QSIM_TRY(probe_passes(cb && setting && flip_mask, c, 3, {tile_bits, tile_low_bits, tile_max_ops, initial_support, false, false, setting}, passes, nullptr, flip_mask));
    return report_schedule(passes, cb, user);
}

extern "C" int qsim_plan_regions_with(const qsim_circuit *c, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support,
                                      const qsim_sched_setting *setting, qsim_pass_region *out, int cap, int *count) {
    std::vector<Pass> passes;
    QSIM_TRY(probe_passes(count && setting && !(cap > 0 && !out), c, 3, {tile_bits, tile_low_bits, tile_max_ops, initial_support, false, true, setting}, passes));
    *count = (int)passes.size();
    fill_regions(c, passes, out, cap);
    return QSIM_OK;
}

// What the planning step's model would choose for this circuit on a state with these options (qsim_choose_schedule without a state):
// every candidate in candidate order with its price, which of them is chosen, and the host seconds the ranking took.
extern "C" int qsim_plan_choice(const qsim_circuit *c, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support, int f32, int with_defer,
                                qsim_sched_setting *out, int cap, int *count, int *chosen, double *seconds) {
    if (!c || !count || !chosen || (cap > 0 && !out)) return fail(QSIM_ERR_ARG, "NULL argument");
    const SchedConfig cfg = engine_sched_config(c->num_q, 3, tile_bits, tile_low_bits, tile_max_ops, 10, f32 != 0, initial_support);
    std::vector<SchedHint> variants;
    std::vector<RankedVariant> ranked;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t best = rank_schedules(cfg, queue_of(c), f32 != 0, with_defer != 0, nullptr, variants, &ranked);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *count = (int)ranked.size(); // (every candidate is evaluated when nothing stops the search: ranked[i] is variants[i])
    *chosen = (int)best;
    for (size_t i = 0; i < ranked.size() && (int)i < cap; i++) out[i] = setting_of(ranked[i].hint, ranked[i].cost, ranked[i].is_default);
    return QSIM_OK;
}

extern "C" int qsim_schedule_circuit(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops,
                                     qsim_sched_cb cb, void *user) {
    std::vector<Pass> passes;
    QSIM_TRY(probe_passes(cb != nullptr, c, fuse, {tile_bits, tile_low_bits, tile_max_ops}, passes));
    return report_schedule(passes, cb, user);
}

extern "C" int qsim_schedule_circuit_from(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support,
                                          qsim_sched_cb cb, void *user) {
    std::vector<Pass> passes;
    QSIM_TRY(probe_passes(cb != nullptr, c, fuse, {tile_bits, tile_low_bits, tile_max_ops, initial_support}, passes));
    return report_schedule(passes, cb, user);
}

extern "C" int qsim_schedule_circuit_deferred(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops,
                                              qsim_sched_cb cb, void *user, uint64_t *flip_mask) {
    std::vector<Pass> passes;
    QSIM_TRY(probe_passes(cb && flip_mask, c, fuse, {tile_bits, tile_low_bits, tile_max_ops, 0, true}, passes, nullptr, flip_mask));
    return report_schedule(passes, cb, user);
}

// The same schedule as the records k_tile would read: every block of every tile pass (the TOP_SCALE factors included) encoded by
// to_tile_op under the pass's geometry, with that geometry, the block's qubits and its matrix beside it.  order_seed != 0: the
// high tile bits of every pass are shuffled first (seeded by it and the pass index), as the engine may reorder them
// (order_tile_bits) — the record then speaks about other tile-local bits while the block stays the same.  What a host-side model
// of the record contract is checked against (tests/tile_record_ref.py).
extern "C" int qsim_tile_records(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops, int f32, uint64_t order_seed,
                                 qsim_tile_record_cb cb, void *user) {
    std::vector<Pass> passes;
    QSIM_TRY(probe_passes(cb != nullptr, c, fuse, {tile_bits, tile_low_bits, tile_max_ops}, passes));
    int pi = 0;
    BlockView view;
    std::vector<TileOp> rec(1); // (zeroed, padding included: the callback is handed its bytes)
    for (const Pass &p : passes) {
        if (p.kclass == QSIM_K_TILE) {
            TileGeom g = p.geom;
            if (order_seed) shuffle_high(g, probe_order_seed(order_seed, (uint64_t)(pi + 1)));
            for (const TileBlock &blk : p.blocks) {
                if (!to_tile_op(g, blk, rec[0], f32 != 0)) return fail(QSIM_ERR_ARG, "internal: block does not fit its tile pass");
                view.set(blk);
                const int geom[3] = {g.tile_bits, g.low_bits, g.n_high};
                cb(user, pi, geom, g.high, blk.s, blk.ns, blk.q, blk.nq, view.matrix.data(), &rec[0], (long)sizeof(TileOp));
            }
        }
        pi++;
    }
    return QSIM_OK;
}
