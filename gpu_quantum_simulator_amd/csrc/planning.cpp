// planning.cpp — everything the engine knows by MEASUREMENT or by trying schedules, and the API that plans without running:
// the tile-bit orders measured per pass geometry ("wisdom") with their file format, the schedule choice per circuit and its
// hints, qsim_tune_circuit*, and the device-free planning calls (qsim_plan_circuit*, qsim_plan_passes, qsim_schedule_circuit,
// qsim_tile_records).
// The three process-wide tables and their locks are private to this file; engine.cpp reaches them through order_tile_bits,
// apply_sched_hint, have_sched_hints and wisdom_epoch (engine_state.h).  Calls the scheduler and, for the timed runs of the
// tuning, the engine's own entry points (qsim_run_circuit, qsim_flush, launch_tile_pass).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>

#include "engine_state.h"

using namespace qsim;

// Which role each high tile bit plays.  Tile-local bit L+j is global bit high[j], in ANY order (the blocks address LDS
// by tile-local bit and are translated through local_bit(), so the order is invisible to them); with 2^L <= 8 amplitudes
// per run and 512 threads, high[0..2] are walked by the lanes of a wave (the 8 runs one load instruction touches),
// high[3..5] by the waves of the workgroup, high[6..8] by the 8 registers of a lane.  The memory-only time of a pass
// depends on this order as much as on the set itself (n = 30, profiles/r02/geom_probe4_fixed_sets.log: one set 6.56 ... 9.05 ms over 48
// random orders, ascending 7.67; another 8.40 ... 14.05, ascending 14.06) and no simple rule predicts it (a boosted-tree
// model on 3000 samples explains a third of the variance), so it is MEASURED: qsim_tune_circuit times candidate
// orders for every pass of a circuit's schedule and keeps the best in a process-wide table keyed by (register size,
// precision, tile shape, bit set) — planning in the sense of FFTW's wisdom, outside any timed region.  Untuned passes
// walk their bits in ascending order (what the scheduler emits).  QSIM_OPT_DEBUG_TILE_ORDER = k > 0 shuffles every
// pass's order with a generator seeded by k and the pass count instead (probes, and the parity tests of the reordering).
struct GeomKey {
    int n, f32, tile_bits, low_bits;
    uint64_t high_mask;
    uint64_t new_mask; // the high bits outside the state's support when the pass starts (0: a pass over a full support).  Such a pass
                       // reads a fraction of what it writes and runs with those bits topmost: another pass than the full one of the same set
    bool operator<(const GeomKey &o) const {
        return std::tie(n, f32, tile_bits, low_bits, high_mask, new_mask) < std::tie(o.n, o.f32, o.tile_bits, o.low_bits, o.high_mask, o.new_mask);
    }
};
struct GeomOrder { int8_t high[kMaxTileHigh]; float ms, ms_ascending; };
static std::mutex g_wisdom_mu;
static std::map<GeomKey, GeomOrder> g_wisdom;
static std::atomic<uint64_t> g_wisdom_epoch{1}; // bumped whenever the table changes: cached plans carry the orders they were built with

static GeomKey geom_key(const qsim_state *s, const TileGeom &g, uint64_t new_mask = 0) {
    GeomKey k{g.n, s->f32 ? 1 : 0, g.tile_bits, g.low_bits, 0, 0};
    for (int j = 0; j < g.n_high; j++) k.high_mask |= 1ULL << g.high[j];
    k.new_mask = new_mask & k.high_mask;
    return k;
}

static void shuffle_high(TileGeom &g, uint64_t seed) {
    uint64_t x = seed | 1ULL;
    for (int i = g.n_high - 1; i > 0; i--) { // Fisher-Yates with xorshift64*
        x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
        const int j = (int)(((x * 0x2545F4914F6CDD1DULL) >> 33) % (uint64_t)(i + 1));
        std::swap(g.high[i], g.high[j]);
    }
}

uint64_t qsim::wisdom_epoch() { return g_wisdom_epoch.load(); }

// The high bits the state is still zero in (new to the support with this pass) go to the top of the order, the others keep
// theirs: the topmost bits are walked by the registers of a lane, and k_tile<SPARSE> then loads only the registers that hold
// something (launch.inc tile_live_regs).  Stable, so placing twice changes nothing.
void qsim::place_new_bits(TileGeom &g, uint64_t zero_mask) {
    std::stable_partition(g.high, g.high + g.n_high, [&](int b) { return !((zero_mask >> b) & 1ULL); });
}

void qsim::order_tile_bits(qsim_state *s, TileGeom &g, uint64_t zero_mask) {
    s->tile_passes++;
    if (g.n_high < 2) return;
    if (s->debug_tile_order > 0) { // any order at all, the new bits wherever they fall: the kernel's other ways of not loading them
        shuffle_high(g, 0x9E3779B97F4A7C15ULL * (uint64_t)(s->debug_tile_order + 1) + 0xD1B54A32D192ED03ULL * s->tile_passes);
        return;
    }
    const uint64_t new_mask = zero_mask & geom_key(s, g).high_mask;
    {
        std::lock_guard<std::mutex> lock(g_wisdom_mu);
        auto it = g_wisdom.find(geom_key(s, g, new_mask));
        if (it != g_wisdom.end())
            for (int j = 0; j < g.n_high; j++) g.high[j] = it->second.high[j];
    }
    place_new_bits(g, new_mask); // (a measured order of this key has them there already)
}

// Scheduler variant per circuit, decided by the planning step (qsim_tune_circuit): key -> SchedConfig::commute.  Circuits
// that were never planned use the default.
// The table is found by key alone: a colliding circuit would be scheduled with another circuit's variant — a valid schedule
// either way (every variant is; the results never depend on it).  Bounded: beyond kMaxSchedHints circuits it starts afresh.
struct SchedHint { int commute; double cheap_margin; int lookahead; int cap; /* clusters per pass; 0: the configuration's own */ uint64_t seed; /* SchedConfig::seed */
                   int defer; /* SchedConfig::defer_flips (the engine still asks whether the flush at hand may: may_defer_flips) */ };
static std::mutex g_hints_mu;
static std::map<uint64_t, SchedHint> g_sched_hints;
constexpr size_t kMaxSchedHints = 4096;
static SchedConfig with_hint(SchedConfig v, const SchedHint &h) {
    v.commute = h.commute; v.cheap_margin = h.cheap_margin; v.lookahead = h.lookahead; v.seed = h.seed; v.defer_flips = h.defer;
    if (h.cap > 0) { v.tile_max_ops = h.cap; v.tail_max_ops = std::max(v.tail_max_ops, h.cap); }
    return v;
}
void qsim::apply_sched_hint(uint64_t key, SchedConfig &cfg) {
    std::lock_guard<std::mutex> lock(g_hints_mu);
    auto it = g_sched_hints.find(key);
    if (it != g_sched_hints.end()) cfg = with_hint(cfg, it->second);
}
bool qsim::have_sched_hints() {
    std::lock_guard<std::mutex> lock(g_hints_mu);
    return !g_sched_hints.empty();
}

struct RankedVariant { SchedHint hint; double cost; bool is_default; };
// circuits whose schedule was chosen by MEASUREMENT (qsim_tune_circuit): the choice stands until the table is cleared — timing
// the same candidates again could flip between near-equal schedules and invalidate the geometries measured for the winner
static std::map<uint64_t, RankedVariant> g_sched_measured; // guarded by g_hints_mu
static void set_sched_hint(uint64_t key, const SchedHint &now, bool is_default, const SchedConfig &scfg) {
    std::lock_guard<std::mutex> lock(g_hints_mu);
    const auto it = g_sched_hints.find(key);
    const SchedHint dflt{scfg.commute, scfg.cheap_margin, scfg.lookahead, 0, 0, 0};
    const SchedHint before = it == g_sched_hints.end() ? dflt : it->second;
    if (is_default) g_sched_hints.erase(key);
    else {
        if (g_sched_hints.size() >= kMaxSchedHints && it == g_sched_hints.end()) { // full: both tables start over together — a measured
            g_sched_hints.clear();                                                // entry without its hint would pin a schedule nobody runs
            const auto mine = g_sched_measured.find(key);
            const bool keep = mine != g_sched_measured.end();
            const RankedVariant kept = keep ? mine->second : RankedVariant{};
            g_sched_measured.clear();
            if (keep) g_sched_measured[key] = kept;
        }
        g_sched_hints[key] = now;
    }
    if (before.commute != now.commute || before.cheap_margin != now.cheap_margin || before.lookahead != now.lookahead || before.cap != now.cap || before.seed != now.seed || before.defer != now.defer)
        g_wisdom_epoch++; // cached plans of this circuit were scheduled another way
}

// The circuit as the gate queue qsim_run_circuit would leave in a state (what the plan and schedule-hint keys are computed from).
static std::vector<QueuedGate> queue_of(const qsim_circuit *c) {
    std::vector<QueuedGate> q;
    q.reserve((size_t)c->count);
    for (long i = 0; i < c->count; i++) q.emplace_back(*c, c->gates[i]);
    return q;
}

// The passes of these gates under this configuration, all at once.
static std::vector<Pass> schedule(const SchedConfig &cfg, const std::vector<QueuedGate> &gates, uint64_t *gates_seen = nullptr) {
    Scheduler sv(cfg);
    feed(sv, gates);
    std::vector<Pass> passes;
    sv.finish(passes);
    if (gates_seen) *gates_seen = sv.gates_seen();
    return passes;
}

// Schedules the circuit under a few dozen scheduler settings, remembers the one whose passes are predicted to take the least
// time (pass_time_cost) under the key qsim_flush will compute for the same gates on a state with this support, and hands its
// passes back.
static void choose_schedule(qsim_state *s, const qsim_circuit *c, const SchedConfig &scfg, std::vector<Pass> *out,
                            std::vector<RankedVariant> *ranked = nullptr, uint64_t *key_out = nullptr, const std::atomic<bool> *stop = nullptr) {
    const std::vector<QueuedGate> q = queue_of(c);
    if (s->fuse < 3) {
        if (out) *out = schedule(scfg, q);
        return;
    }
    const uint64_t key = gates_key(s, plan_identity(s, q.size(), scfg.initial_support), q.data(), q.size());
    if (key_out) *key_out = key;
    {
        // A circuit whose schedule was chosen by measurement keeps it: no candidate is scheduled again (80 schedules cost about a
        // second at n = 30), and the hint is put back in case the hint table was emptied in between (kMaxSchedHints) — without
        // it the circuit would silently run its default schedule with the geometries measured for another one.
        bool measured = false;
        RankedVariant kept{};
        {
            std::lock_guard<std::mutex> lock(g_hints_mu);
            auto it = g_sched_measured.find(key);
            if (it != g_sched_measured.end()) { measured = true; kept = it->second; }
        }
        if (measured) {
            set_sched_hint(key, kept.hint, kept.is_default, scfg);
            if (ranked) ranked->clear(); // nothing left to try
            if (out) *out = schedule(with_hint(scfg, kept.hint), q);
            return;
        }
    }
    // the variants: how many clusters a pass may take (where the engine sets a cap of its own: states of 4 GiB and more),
    // clusters may / may not overtake (commute), how eagerly passes inside the support are kept (cheap_margin), one more
    // pass of lookahead where the local search is on; the default comes first and wins ties
    std::vector<SchedHint> variants;
    std::vector<int> caps{0};
    if (scfg.tail_max_ops > scfg.tile_max_ops) // the engine's own cap is in force (engine_sched_config), not a caller's
        for (int cap : {24, 28, 32, 40})
            if (cap != scfg.tile_max_ops) caps.push_back(cap);
    // (commuting clusters first: over 16 seeded 1000-gate circuits at n = 30 a schedule without them never came within 15 % of the best
    // of these candidates, so a search that is cut short — `stop` — spends its time on the half that wins)
    for (int com = 1; com >= 0; com--)
        for (int cap : caps)
            for (double mar : {scfg.cheap_margin, 2.0 * scfg.cheap_margin})
                for (int la = scfg.lookahead; la <= scfg.lookahead + (scfg.lookahead >= 1 ? 1 : 0); la++) variants.push_back({com, mar, la, cap, 0, 0});
    // ... and every one of them with the X gates left to the stores of the last tile pass (SchedConfig::defer_flips), where a flush
    // of this state may do that.  Fewer qubits are forced into tiles, but the greedy packing does not gain from it on every circuit.
    // (Not on the cold path: the second buffer that out-of-place passes need cannot be asked for while the first is being allocated.)
    if (!stop && s->defer_flips != 0 && may_defer_flips(s))
        for (size_t vi = 0, nv = variants.size(); vi < nv; vi++) {
            SchedHint h = variants[vi];
            h.defer = 1;
            variants.push_back(h);
        }
    // Every candidate is an independent run of the scheduler on the same gates: they are evaluated on up to 16 host threads
    // (80 schedules at n = 30: 0.9-1.3 s on one thread) and REDUCED in candidate order with the same rule as before — the default
    // first, a later one only when it is at least 0.5 % cheaper — so the choice does not depend on the thread count.  `stop`
    // (the cold path of the C host: "plan while the state is being allocated, no longer") ends the search early: candidates not
    // evaluated by then simply do not take part; the default always does.
    std::vector<double> costs; // per candidate; < 0: not evaluated
    auto evaluate = [&](size_t first, size_t last) {
        costs.resize(last, -1.0);
        std::atomic<size_t> next{first};
        auto worker = [&]() {
            for (;;) {
                const size_t vi = next.fetch_add(1);
                if (vi >= last) return;
                if (vi != 0 && stop && stop->load()) return;
                Scheduler sv(with_hint(scfg, variants[vi]));
                feed(sv, q);
                double cost = 0;
                sv.finish([&](Pass &&p) { cost += pass_time_cost(p, s->f32); });
                costs[vi] = cost;
            }
        };
        const unsigned hw = std::thread::hardware_concurrency();
        const size_t nthreads = std::min<size_t>({(size_t)16, (size_t)(hw ? hw : 1), last - first}); // a GPU's share of its host's cores
        std::vector<std::thread> pool;
        for (size_t t = 1; t < nthreads; t++) pool.emplace_back(worker);
        worker();
        for (std::thread &t : pool) t.join();
    };
    double best_cost = 0;
    size_t best = 0;
    auto reduce = [&](size_t first, size_t last) {
        for (size_t vi = first; vi < last; vi++) {
            if (costs[vi] < 0) continue;
            if (ranked) ranked->push_back({variants[vi], costs[vi], vi == 0});
            if (vi == 0 || costs[vi] < best_cost * 0.995) { best_cost = costs[vi]; best = vi; }
        }
    };
    evaluate(0, variants.size());
    reduce(0, variants.size());
    // ... and, for the three settings that came out best, the same setting with its ties broken differently (SchedConfig::seed):
    // the greedy packing is sensitive to which of several equally good clusters or qubits it takes first — over 40 seeds the
    // swept bytes of one setting spread by 10 % and more (bench circuit 9.57 -> 8.63 sweeps, another 9.13 -> 8.06)
    if ((variants.size() > 1 || scfg.local_iters > 0) && !(stop && stop->load())) {
        std::vector<size_t> order;
        for (size_t i = 0; i < variants.size(); i++)
            if (costs[i] >= 0) order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return costs[a] < costs[b]; });
        const size_t base_count = std::min<size_t>(3, order.size()), first_seeded = variants.size();
        constexpr int kSeeds = 16;
        for (size_t b = 0; b < base_count; b++)
            for (int sd = 1; sd <= kSeeds; sd++) {
                SchedHint h = variants[order[b]];
                h.seed = (uint64_t)sd;
                variants.push_back(h);
            }
        evaluate(first_seeded, variants.size());
        reduce(first_seeded, variants.size());
    }
    set_sched_hint(key, variants[best], best == 0, scfg);
    if (out) *out = schedule(with_hint(scfg, variants[best]), q); // one more run of the scheduler: the candidates kept their costs only
}

// The schedule choice alone (no timing): for a run from a reset and for a run on a dense state.
extern "C" int qsim_choose_schedule(qsim_state *s, const qsim_circuit *c) {
    QSIM_TRY(check_circuit(s, c));
    QSIM_TRY(qsim_flush(s));
    for (int dense = 0; dense < 2; dense++) {
        if (!dense && !s->sparse_start) continue;
        const SchedConfig scfg = state_sched_config(s, dense ? ~0ULL : 0);
        choose_schedule(s, c, scfg, nullptr);
    }
    return QSIM_OK;
}

// The cold path of the C host (bin/qsim: one circuit, one run, quantum_simulator.c:143-248): the schedule choice for a run from a
// reset, for as long as the state's buffer is still being allocated (qsim_create_async) and no longer — the candidates evaluated
// by then compete, the default always does.  With a buffer that is already there it returns at once with the default schedule.
extern "C" int qsim_choose_schedule_while_allocating(qsim_state *s, const qsim_circuit *c) {
    QSIM_TRY(check_circuit(s, c));
    if (s->alloc_done.load() || s->fuse < 3) return QSIM_OK;
    const SchedConfig scfg = state_sched_config(s, s->sparse_start ? 0 : ~0ULL);
    { // the tile kernel's code object is loaded at its first use: here, beside the allocation, instead of in front of the first pass
        HIP_TRY(hipSetDevice(s->device));
        TileGeom g{};
        g.tile_bits = std::min(scfg.tile_bits, s->n);
        g.low_bits = std::min(scfg.tile_low_bits, g.tile_bits);
        g.n_high = g.tile_bits - g.low_bits;
        g.n = s->n;
        LaunchCfg cfg{s->stream, s->grid_cap, true};
        (void)launch_tile(cfg, nullptr, nullptr, s->f32, g, nullptr, 0, s->tile_threads, false, 1.0);
        (void)hipGetLastError();
    }
    choose_schedule(s, c, scfg, nullptr, nullptr, nullptr, &s->alloc_done);
    return QSIM_OK;
}

// The same choice for a run that finds the state with exactly this support (what qsim_flush will key its lookup with: all ones
// for a dense state, 0 fresh from a reset, the mask of qsim_set_support after a sparse exchange).
extern "C" int qsim_choose_schedule_for(qsim_state *s, const qsim_circuit *c, uint64_t support) {
    QSIM_TRY(check_circuit(s, c));
    QSIM_TRY(qsim_flush(s));
    choose_schedule(s, c, state_sched_config(s, plan_support(s, support)), nullptr);
    return QSIM_OK;
}

// Where a state that has this support can be non-zero after the circuit, as THIS engine will know it then: the circuit is
// scheduled the way qsim_flush will schedule the same gates (same options, same remembered schedule choice) and every tile pass
// adds its tile qubits; a single-gate kernel makes the state dense.  A cluster's planner derives from it what an exchange's
// receivers look at, so that the sender's last tile pass — which writes exactly this — can do the re-layout itself.
extern "C" int qsim_support_after(qsim_state *s, const qsim_circuit *c, uint64_t support, uint64_t *after) {
    if (!after) return fail(QSIM_ERR_ARG, "NULL argument");
    QSIM_TRY(check_circuit(s, c));
    const uint64_t nmask = index_mask(s->n);
    if (!s->sparse_start || (support & nmask) == nmask) { *after = nmask; return QSIM_OK; }
    support &= nmask;
    if (c->count == 0) { *after = support; return QSIM_OK; }
    SchedConfig scfg = state_sched_config(s, support);
    const std::vector<QueuedGate> q = queue_of(c);
    if (s->fuse >= 3 && have_sched_hints()) apply_sched_hint(gates_key(s, plan_identity(s, q.size(), support), q.data(), q.size()), scfg);
    scfg.defer_flips = (s->defer_flips == 2 || (s->defer_flips == 1 && scfg.defer_flips)) && may_defer_flips(s) ? 1 : 0; // as qsim_flush decides (a shard never defers)
    Scheduler sv(scfg);
    feed(sv, q);
    uint64_t sup = support | sv.residual_flips(); // a flipped qubit is inside the support afterwards, whichever pass applies the flip
    sv.finish([&](Pass &&p) {
        if (p.kclass != QSIM_K_TILE) { sup = nmask; return; } // the engine writes the zeros out first (materialize_zero_ket)
        sup |= tile_mask(p.geom);
    });
    *after = sup & nmask;
    return QSIM_OK;
}

// ---- measured pass geometry -------------------------------------------------------------------------------------------
// Plans the circuit exactly as qsim_run_circuit + qsim_flush would and, for every tile pass whose geometry is not in the
// table yet, times the pass (its real blocks, on whatever the state buffer holds) under candidate orders of its high
// tile bits: ascending first, then pseudo-random permutations seeded by the bit set, until max_candidates have been
// tried or the pass's share of budget_ms is spent (at least four).  The fastest order goes into the process-wide table
// order_tile_bits() consults.  The state's contents are clobbered, so it is left reset to |0...0>.  Results never
// depend on the order; only the pass times do.
extern "C" int qsim_tune_circuit(qsim_state *s, const qsim_circuit *c, int max_candidates, double budget_ms, qsim_tune_report *rep) {
    return qsim_tune_circuit_from(s, c, max_candidates, budget_ms, rep, 0);
}

extern "C" int qsim_tune_circuit_from(qsim_state *s, const qsim_circuit *c, int max_candidates, double budget_ms, qsim_tune_report *rep,
                                      int dense_start) {
    return qsim_tune_circuit_support(s, c, max_candidates, budget_ms, rep, dense_start ? ~0ULL : 0);
}

// The model is good to ~0.4 ms per pass, i.e. it cannot tell schedules apart that differ by less than ~2 %: the schedules it
// likes best (distinct predicted costs, QSIM_TUNE_SCHEDULES of them) are RUN once each on the state and the fastest is kept
// as the circuit's measured choice; `passes` receives its passes.
static int keep_fastest_schedule(qsim_state *s, const qsim_circuit *c, const SchedConfig &scfg, uint64_t support, uint64_t sched_key,
                                 std::vector<RankedVariant> &ranked, std::vector<Pass> &passes) {
    std::stable_sort(ranked.begin(), ranked.end(), [](const RankedVariant &a, const RankedVariant &b) { return a.cost < b.cost; });
    std::vector<RankedVariant> tries;
    if (const char *v = getenv("QSIM_TUNE_SCHEDULES")) s->tune_schedules = std::max(1, std::min(80, atoi(v)));
    // ... of the schedules without deferred X gates and of those with them alike: the model prices the flipping pass like any other and
    // ranks the two families against each other only roughly, so the best of the first family is always among the ones run
    for (int defer = 0; defer < 2; defer++) {
        size_t taken = 0;
        for (const RankedVariant &v : ranked) { // distinct predicted costs = (almost surely) distinct schedules
            if (v.hint.defer != defer) continue;
            bool dup = false;
            for (const RankedVariant &t : tries) dup = dup || t.cost == v.cost;
            if (!dup) { tries.push_back(v); taken++; }
            if (taken == (size_t)s->tune_schedules) break;
        }
    }
    hipEvent_t t0 = nullptr, t1 = nullptr;
    HIP_TRY(hipEventCreate(&t0));
    HIP_TRY(hipEventCreate(&t1));
    const int saved_profile = s->profile;
    s->profile = 0;
    const uint64_t nmask = index_mask(s->n);
    float best_ms = 0.f;
    size_t best_i = 0;
    int rc = QSIM_OK;
    for (size_t i = 0; i < tries.size() && rc == QSIM_OK; i++) {
        set_sched_hint(sched_key, tries[i].hint, tries[i].is_default, scfg);
        float ms = 0.f;
        for (int rep2 = 0; rep2 < 2 && rc == QSIM_OK; rep2++) { // the second run replays the cached plan: no host work in the way
            if (support == 0) rc = qsim_reset(s);
            else if (support != ~0ULL) rc = qsim_set_support(s, support & nmask);
            else { s->zero_ket_pending = false; s->partial = false; } // a dense state: whatever the buffer holds
            if (rc) break;
            (void)hipEventRecord(t0, s->stream);
            rc = qsim_run_circuit(s, c, 0, -1);
            if (rc == QSIM_OK) rc = qsim_flush(s);
            (void)hipEventRecord(t1, s->stream);
            if (rc == QSIM_OK && hipEventSynchronize(t1) != hipSuccess) rc = fail(QSIM_ERR_DEVICE, "planning: event sync failed");
            if (rc == QSIM_OK && hipEventElapsedTime(&ms, t0, t1) != hipSuccess) rc = fail(QSIM_ERR_DEVICE, "planning: event time failed");
        }
        if (i == 0 || ms < best_ms) { best_ms = ms; best_i = i; }
    }
    s->profile = saved_profile;
    s->stats.gates -= std::min<uint64_t>(s->stats.gates, (uint64_t)c->count * 2 * tries.size()); // planning runs are not gate statements of the caller
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    if (rc) return rc;
    set_sched_hint(sched_key, tries[best_i].hint, tries[best_i].is_default, scfg);
    {
        std::lock_guard<std::mutex> lock(g_hints_mu);
        if (g_sched_measured.size() >= kMaxSchedHints) g_sched_measured.clear();
        g_sched_measured[sched_key] = tries[best_i];
    }
    passes = schedule(with_hint(scfg, tries[best_i].hint), queue_of(c)); // the schedule that won: its tile-bit orders are measured next
    return qsim_sync(s);
}

// Times every tile pass of `passes` whose geometry is not in the table yet under candidate orders of its high bits and enters
// the fastest (qsim_tune_circuit's comment).  The state's contents are scratch here; the buffers keep their roles.
// support: where the state can be non-zero when the first pass starts (0: a reset, ~0: dense).  A pass over a partial support is
// timed as it will run — on that support, its new bits topmost in every candidate — and entered under a key of its own.
static int measure_tile_orders(qsim_state *s, const std::vector<Pass> &passes, uint64_t support, int max_candidates, double budget_ms, qsim_tune_report &r) {
    struct Todo { const Pass *p; uint64_t zero_mask, new_mask; };
    std::vector<Todo> todo;
    const uint64_t nmask = index_mask(s->n);
    for (const Pass &p : passes) {
        if (p.kclass != QSIM_K_TILE) { support = ~0ULL; continue; } // any other kernel works on a materialised state
        uint64_t zero_mask = 0;
        if ((support & nmask) != nmask) {
            if ((support & nmask) != 0) zero_mask = nmask & ~support; // (the generating pass reads nothing: its order is the full pass's)
            support |= tile_mask(p.geom);
        }
        r.tile_passes++;
        if (p.geom.n_high < 2) continue;
        const GeomKey key = geom_key(s, p.geom, zero_mask);
        std::lock_guard<std::mutex> lock(g_wisdom_mu);
        if (g_wisdom.count(key)) { r.already_known++; continue; }
        bool dup = false;
        for (const Todo &q : todo) dup = dup || (geom_key(s, q.p->geom).high_mask == key.high_mask && q.new_mask == key.new_mask);
        if (!dup) todo.push_back({&p, zero_mask, key.new_mask});
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    const auto t_begin = std::chrono::steady_clock::now();
    auto elapsed_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    void *const home = s->amps;
    const bool tune_oop = !todo.empty() && spare_buffer(s) != nullptr;
    uint64_t zero_mask = 0;
    auto timed = [&](const Pass &p, const TileGeom &g, float &ms) -> int {
        (void)hipEventRecord(e0, s->stream);
        const int rc2 = launch_tile_pass(s, p, g, false, nullptr, tune_oop, zero_mask); // timed the way most passes of a run go
        if (rc2) return rc2;
        (void)hipEventRecord(e1, s->stream);
        if (hipEventSynchronize(e1) != hipSuccess) return fail(QSIM_ERR_DEVICE, "tuning: event sync failed");
        if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return fail(QSIM_ERR_DEVICE, "tuning: event time failed");
        return QSIM_OK;
    };
    int rc = QSIM_OK;
    for (size_t i = 0; i < todo.size() && rc == QSIM_OK; i++) {
        const Pass &p = *todo[i].p;
        zero_mask = todo[i].zero_mask;
        const double share_end = budget_ms > 0 ? budget_ms * (double)(i + 1) / (double)todo.size() : 1e300;
        TileGeom asc = p.geom;
        std::sort(asc.high, asc.high + asc.n_high);
        place_new_bits(asc, todo[i].new_mask); // "ascending" for a partial pass: what it runs with when nothing is measured
        float ms = 0.f;
        rc = timed(p, asc, ms); // warm: first touch of the op buffer and of this geometry's code path
        if (rc == QSIM_OK) rc = timed(p, asc, ms);
        if (rc) break;
        GeomOrder best{};
        for (int j = 0; j < asc.n_high; j++) best.high[j] = (int8_t)asc.high[j];
        best.ms = best.ms_ascending = ms;
        const GeomKey key = geom_key(s, asc, todo[i].new_mask);
        for (int cand = 1; cand < max_candidates; cand++) {
            if (cand >= 4 && elapsed_ms() > share_end) break;
            TileGeom g = asc;
            std::sort(g.high, g.high + g.n_high);
            shuffle_high(g, key.high_mask * 0x9E3779B97F4A7C15ULL + (uint64_t)cand * 0xD1B54A32D192ED03ULL);
            place_new_bits(g, key.new_mask);
            rc = timed(p, g, ms);
            if (rc) break;
            r.candidates_timed++;
            if (ms < best.ms) {
                best.ms = ms;
                for (int j = 0; j < g.n_high; j++) best.high[j] = (int8_t)g.high[j];
            }
        }
        if (rc) break;
        if (best.ms < best.ms_ascending * 0.985f) { // keep ascending unless the gain is beyond the timing noise
            r.passes_reordered++;
        } else {
            for (int j = 0; j < asc.n_high; j++) best.high[j] = (int8_t)asc.high[j];
            best.ms = best.ms_ascending;
        }
        r.ms_ascending += best.ms_ascending;
        r.ms_best += best.ms;
        r.passes_tuned++;
        std::lock_guard<std::mutex> lock(g_wisdom_mu);
        g_wisdom[key] = best;
        g_wisdom_epoch++;
    }
    (void)hipStreamSynchronize(s->stream);
    if (s->amps != home) std::swap(s->amps, s->spare); // contents are scratch here (reset below); the buffers keep their roles
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    r.seconds = elapsed_ms() * 1e-3;
    return rc;
}

extern "C" int qsim_tune_circuit_support(qsim_state *s, const qsim_circuit *c, int max_candidates, double budget_ms, qsim_tune_report *rep, uint64_t support) {
    QSIM_TRY(check_circuit(s, c));
    if (max_candidates < 1) max_candidates = 1;
    QSIM_TRY(qsim_sync(s));
    HIP_TRY(hipSetDevice(s->device));
    support = plan_support(s, support);
    SchedConfig scfg = state_sched_config(s, support); // 0: the run that follows starts from the reset this call ends with
    // Which way to schedule THIS circuit is decided first; its passes are the ones measured below.  The pass-time model ranks
    // the scheduler settings (choose_schedule); with timing allowed (max_candidates > 1) the ones it likes best are then run.
    std::vector<Pass> passes;
    std::vector<RankedVariant> ranked;
    uint64_t sched_key = 0;
    choose_schedule(s, c, scfg, &passes, &ranked, &sched_key);
    if (max_candidates > 1 && s->fuse >= 3 && ranked.size() > 1)
        QSIM_TRY(keep_fastest_schedule(s, c, scfg, support, sched_key, ranked, passes));
    qsim_tune_report r{};
    const int rc = measure_tile_orders(s, passes, support, max_candidates, budget_ms, r);
    if (rep) *rep = r;
    const int rc_reset = qsim_reset(s);
    return rc ? rc : rc_reset;
}

extern "C" long qsim_tune_table_size(void) {
    std::lock_guard<std::mutex> lock(g_wisdom_mu);
    return (long)g_wisdom.size();
}

// The table as text, one geometry per line: [part new_mask(hex)] n f32 tile_bits low_bits high_mask(hex) ms ms_ascending order...  A table
// measured once (per machine) can be loaded by later processes: the C host does so when QSIM_WISDOM names a file.
extern "C" int qsim_tune_table_save(const char *path) {
    if (!path) return fail(QSIM_ERR_ARG, "NULL path");
    FILE *f = fopen(path, "w");
    if (!f) return fail(QSIM_ERR_OPEN, "cannot write %s", path);
    {   // measured schedule choices: "sched <key> <commute> <cheap_margin> <lookahead> <cap> <is_default>"
        std::lock_guard<std::mutex> lock(g_hints_mu);
        for (const auto &kv : g_sched_measured)
            fprintf(f, "sched %llx %d %.17g %d %d %d %llu%s\n", (unsigned long long)kv.first, kv.second.hint.commute, kv.second.hint.cheap_margin,
                    kv.second.hint.lookahead, kv.second.hint.cap, kv.second.is_default ? 1 : 0, (unsigned long long)kv.second.hint.seed,
                    kv.second.hint.defer ? " 1" : ""); // an eighth field only where X gates are deferred: other lines stay what older files hold
    }
    std::lock_guard<std::mutex> lock(g_wisdom_mu);
    for (const auto &kv : g_wisdom) {
        const int nh = __builtin_popcountll(kv.first.high_mask);
        if (kv.first.new_mask) fprintf(f, "part %llx ", (unsigned long long)kv.first.new_mask); // a pass over a partial support
        fprintf(f, "%d %d %d %d %llx %.4f %.4f", kv.first.n, kv.first.f32, kv.first.tile_bits, kv.first.low_bits,
                (unsigned long long)kv.first.high_mask, kv.second.ms, kv.second.ms_ascending);
        for (int j = 0; j < nh; j++) fprintf(f, " %d", (int)kv.second.high[j]);
        fprintf(f, "\n");
    }
    fclose(f);
    return QSIM_OK;
}

extern "C" long qsim_tune_table_load(const char *path) {
    if (!path) return -1;
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    long loaded = 0;
    char line[512];
    while (fgets(line, sizeof line, f)) {
        if (strncmp(line, "sched ", 6) == 0) {
            unsigned long long key = 0, seed = 0;
            RankedVariant rv{};
            int isd = 0;
            if (sscanf(line + 6, "%llx %d %lf %d %d %d %llu %d", &key, &rv.hint.commute, &rv.hint.cheap_margin, &rv.hint.lookahead, &rv.hint.cap, &isd, &seed, &rv.hint.defer) >= 6 &&
                (rv.hint.defer == 0 || rv.hint.defer == 1) &&
                rv.hint.cheap_margin > 0 && rv.hint.lookahead >= 0 && rv.hint.lookahead <= 8 && rv.hint.cap >= 0 && rv.hint.cap <= 512) {
                rv.is_default = isd != 0;
                rv.hint.seed = seed;
                std::lock_guard<std::mutex> lock(g_hints_mu);
                g_sched_measured[key] = rv;
                if (rv.is_default) g_sched_hints.erase(key); else g_sched_hints[key] = rv.hint;
                g_wisdom_epoch++;
                loaded++;
            }
            continue;
        }
        GeomKey k{};
        GeomOrder o{};
        unsigned long long hm = 0, nm = 0;
        int used = 0, skip = 0;
        // "part <new_mask>" in front: the order of a pass that admits those bits to the support.  Lines without it (every line of
        // a file written before such passes were told apart) are orders of full passes and are looked up for those alone.
        if (strncmp(line, "part ", 5) == 0 && (sscanf(line + 5, "%llx %n", &nm, &skip) < 1 || nm == 0)) continue;
        if (nm) memmove(line, line + 5 + skip, strlen(line + 5 + skip) + 1);
        if (sscanf(line, "%d %d %d %d %llx %f %f%n", &k.n, &k.f32, &k.tile_bits, &k.low_bits, &hm, &o.ms, &o.ms_ascending, &used) < 7) continue;
        k.high_mask = hm;
        k.new_mask = nm;
        const int nh = __builtin_popcountll(hm);
        if (nh < 2 || nh > kMaxTileHigh || (nm & ~hm)) continue;
        const char *p = line + used;
        uint64_t seen = 0;
        bool ok = true;
        for (int j = 0; j < nh && ok; j++) {
            int v = -1, adv = 0;
            if (sscanf(p, "%d%n", &v, &adv) < 1 || v < 0 || v > 62 || !((hm >> v) & 1ULL) || ((seen >> v) & 1ULL)) ok = false;
            else { o.high[j] = (int8_t)v; seen |= 1ULL << v; p += adv; }
        }
        if (!ok) continue; // not a permutation of the set: ignore the line
        for (int j = 0, seen_new = 0; j < nh && ok; j++) { // the new bits topmost, as the engine runs such a pass
            const bool is_new = (nm >> o.high[j]) & 1ULL;
            if (seen_new && !is_new) ok = false;
            seen_new |= is_new;
        }
        if (!ok) continue;
        std::lock_guard<std::mutex> lock(g_wisdom_mu);
        g_wisdom[k] = o;
        g_wisdom_epoch++;
        loaded++;
    }
    fclose(f);
    return loaded;
}

extern "C" void qsim_tune_table_clear(void) {
    {
        std::lock_guard<std::mutex> lock(g_hints_mu);
        g_sched_hints.clear();
        g_sched_measured.clear();
    }
    std::lock_guard<std::mutex> lock(g_wisdom_mu);
    g_wisdom.clear();
    g_wisdom_epoch++;
}

extern "C" int qsim_plan_circuit(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, qsim_stats *out) {
    return qsim_plan_circuit_from(c, fuse, tile_bits, tile_low_bits, 0, out);
}

extern "C" int qsim_plan_circuit_from(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, uint64_t initial_support, qsim_stats *out) {
    if (!c || !out) return fail(QSIM_ERR_ARG, "NULL argument");
    if (fuse < 0 || fuse > 3) return fail(QSIM_ERR_ARG, "fuse level %d not in 0..3", fuse);
    memset(out, 0, sizeof *out);
    const std::vector<Pass> passes = schedule(engine_sched_config(c->num_q, fuse, tile_bits, tile_low_bits, 32, 10, false, initial_support), queue_of(c), &out->gates);
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
    if (!c || !count || (cap > 0 && !out)) return fail(QSIM_ERR_ARG, "NULL argument");
    if (fuse < 0 || fuse > 3) return fail(QSIM_ERR_ARG, "fuse level %d not in 0..3", fuse);
    const std::vector<Pass> passes = schedule(engine_sched_config(c->num_q, fuse, tile_bits, tile_low_bits, 32, 10, false, initial_support), queue_of(c));
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

static int report_schedule(const std::vector<Pass> &passes, qsim_sched_cb cb, void *user);

extern "C" int qsim_schedule_circuit(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops,
                                     qsim_sched_cb cb, void *user) {
    if (!c || !cb) return fail(QSIM_ERR_ARG, "NULL argument");
    if (fuse < 0 || fuse > 3) return fail(QSIM_ERR_ARG, "fuse level %d not in 0..3", fuse);
    return report_schedule(schedule(engine_sched_config(c->num_q, fuse, tile_bits, tile_low_bits, tile_max_ops), queue_of(c)), cb, user);
}

extern "C" int qsim_schedule_circuit_deferred(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops,
                                              qsim_sched_cb cb, void *user, uint64_t *flip_mask) {
    if (!c || !cb || !flip_mask) return fail(QSIM_ERR_ARG, "NULL argument");
    if (fuse < 0 || fuse > 3) return fail(QSIM_ERR_ARG, "fuse level %d not in 0..3", fuse);
    SchedConfig cfg = engine_sched_config(c->num_q, fuse, tile_bits, tile_low_bits, tile_max_ops);
    cfg.defer_flips = 1;
    Scheduler sv(cfg);
    feed(sv, queue_of(c));
    std::vector<Pass> passes;
    sv.finish(passes);
    *flip_mask = sv.residual_flips();
    return report_schedule(passes, cb, user);
}

static int report_schedule(const std::vector<Pass> &passes, qsim_sched_cb cb, void *user) {
    int pi = 0;
    std::vector<double> big((size_t)2 * 256 * 256);
    std::vector<cd> full((size_t)256 * 256);
    for (const Pass &p : passes) {
        for (const FusedOp &op : p.ops) {
            double U[128];
            const int d = op.kind == OP_CX ? 0 : op.dim();
            for (int k = 0; k < d * d; k++) { U[2 * k] = op.m[k].real(); U[2 * k + 1] = op.m[k].imag(); }
            const int kind = op.kind == OP_G1 ? QSIM_GATE_U1 : op.kind == OP_CX ? QSIM_GATE_CX : QSIM_GATE_U2;
            const int qs[2] = {op.q_hi, op.q_lo};
            cb(user, pi, p.kclass, kind, qs, op.kind == OP_CX ? 2 : op.nq(), d ? U : nullptr, (int)op.gates);
        }
        for (const TileBlock &blk : p.blocks) { // reported as ONE matrix on (selecting qubits..., tile qubits...)
            TileOp t;
            if (!to_tile_op(p.geom, blk, t)) return fail(QSIM_ERR_ARG, "internal: block does not fit its tile pass");
            const int nq = blk.ns + blk.nq, D = 1 << nq;
            blk.full_matrix(full.data());
            for (int k = 0; k < D * D; k++) { big[2 * k] = full[k].real(); big[2 * k + 1] = full[k].imag(); }
            int qs[kMaxBlockQ + 2], j = 0;
            for (int a = 0; a < blk.ns; a++) qs[j++] = blk.s[a];
            for (int a = 0; a < blk.nq; a++) qs[j++] = blk.q[a];
            static const int kinds[9] = {0, QSIM_GATE_U1, QSIM_GATE_U2, QSIM_GATE_U3, QSIM_GATE_U4, QSIM_GATE_U5, QSIM_GATE_U6, QSIM_GATE_U7, QSIM_GATE_U8};
            cb(user, pi, p.kclass, kinds[nq], qs, nq, big.data(), (int)blk.gates);
        }
        pi++;
    }
    return QSIM_OK;
}

// The same schedule as the records k_tile would read: every block of every tile pass (the TOP_SCALE factors included) encoded by
// to_tile_op under the pass's geometry, with that geometry, the block's qubits and its matrix beside it.  order_seed != 0: the
// high tile bits of every pass are shuffled first (seeded by it and the pass index), as the engine may reorder them
// (order_tile_bits) — the record then speaks about other tile-local bits while the block stays the same.  What a host-side model
// of the record contract is checked against (tests/tile_record_ref.py).
extern "C" int qsim_tile_records(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops, int f32, uint64_t order_seed,
                                 qsim_tile_record_cb cb, void *user) {
    if (!c || !cb) return fail(QSIM_ERR_ARG, "NULL argument");
    if (fuse < 0 || fuse > 3) return fail(QSIM_ERR_ARG, "fuse level %d not in 0..3", fuse);
    const std::vector<Pass> passes = schedule(engine_sched_config(c->num_q, fuse, tile_bits, tile_low_bits, tile_max_ops), queue_of(c));
    int pi = 0;
    std::vector<double> big((size_t)2 * 256 * 256);
    std::vector<cd> full((size_t)256 * 256);
    std::vector<TileOp> rec(1);
    for (const Pass &p : passes) {
        if (p.kclass == QSIM_K_TILE) {
            TileGeom g = p.geom;
            if (order_seed) shuffle_high(g, 0x9E3779B97F4A7C15ULL * (order_seed + 1) + 0xD1B54A32D192ED03ULL * (uint64_t)(pi + 1));
            for (const TileBlock &blk : p.blocks) {
                if (!to_tile_op(g, blk, rec[0], f32 != 0)) return fail(QSIM_ERR_ARG, "internal: block does not fit its tile pass");
                const int D = 1 << (blk.ns + blk.nq);
                blk.full_matrix(full.data());
                for (int k = 0; k < D * D; k++) { big[2 * k] = full[k].real(); big[2 * k + 1] = full[k].imag(); }
                const int geom[3] = {g.tile_bits, g.low_bits, g.n_high};
                cb(user, pi, geom, g.high, blk.s, blk.ns, blk.q, blk.nq, big.data(), &rec[0], (long)sizeof(TileOp));
            }
        }
        pi++;
    }
    return QSIM_OK;
}
