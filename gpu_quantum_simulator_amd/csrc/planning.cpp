// planning.cpp — the planning step on a state: which way to schedule a circuit, by the pass-time model (choose_schedule, the
// qsim_choose_schedule* entry points) and where timing is allowed by running the best candidates (qsim_tune_circuit*), which also
// measures the tile-bit orders of the winner's passes; and qsim_support_after, which says what a flush will leave.
// What it learns goes into the tables of wisdom.cpp (planning.h).  Calls the scheduler, the engine's flush rule (flush_rule) and,
// for the timed runs, the engine's own entry points (qsim_run_circuit, qsim_flush, launch_tile_pass).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <thread>

#include "planning.h"

using namespace qsim;

// The candidates of the planning step and their prices: the circuit scheduled under a few dozen to a few hundred scheduler settings,
// each priced by the pass-time model.  Needs no state: `f32` and `with_defer` (a flush of the state may leave X gates to the last
// pass's stores) say what it has to know of one.  Returns the index of the choice in `variants` (0: the default).
size_t qsim::rank_schedules(const SchedConfig &scfg, const std::vector<QueuedGate> &q, bool f32, bool with_defer, const std::atomic<bool> *stop,
                            std::vector<SchedHint> &variants, std::vector<RankedVariant> *ranked) {
    // the variants: how many clusters a pass may take (where the engine sets a cap of its own: states of 4 GiB and more),
    // clusters may / may not overtake (commute), how eagerly passes inside the support are kept (cheap_margin), one more
    // pass of lookahead where the local search is on; the default comes first and wins ties
    variants.clear();
    std::vector<int> caps{0};
    if (scfg.tail_max_ops > scfg.tile_max_ops) // the engine's own cap is in force (engine_sched_config), not a caller's
        for (int cap : {24, 28, 32, 40})
            if (cap != scfg.tile_max_ops) caps.push_back(cap);
    // (commuting clusters first: over 16 seeded 1000-gate circuits at n = 30 a schedule without them never came within 15 % of the best
    // of these candidates, so a search that is cut short — `stop` — spends its time on the half that wins)
    for (int com = 1; com >= 0; com--)
        for (int cap : caps)
            for (double mar : {scfg.cheap_margin, 2.0 * scfg.cheap_margin})
                for (int la = scfg.lookahead; la <= scfg.lookahead + (scfg.lookahead >= 1 ? 1 : 0); la++) variants.push_back({com, mar, la, cap, 0, 0, 0});
    // ... and every one of them with the X gates left to the stores of the last tile pass (SchedConfig::defer_flips), where a flush
    // of this state may do that.  Fewer qubits are forced into tiles, but the greedy packing does not gain from it on every circuit.
    if (with_defer)
        for (size_t vi = 0, nv = variants.size(); vi < nv; vi++) {
            SchedHint h = variants[vi];
            h.defer = 1;
            variants.push_back(h);
        }
    // A run that starts on a partial support and has the time (not the cold path, which keeps the candidates above) plans over how the
    // support grows as well: passes inside the support kept twice as eagerly (cheap_margin x 0.5), and every variant with the packer
    // weighing the support's growth (SchedConfig::support_weight 5 and 10).  On the bench circuit the schedules with four full sweeps
    // instead of five are only found with a weight.  The candidates above stay first, in their order.
    const bool partial_start = !stop && (scfg.initial_support & index_mask(scfg.n)) != index_mask(scfg.n);
    if (partial_start) {
        for (size_t vi = 0, nv = variants.size(); vi < nv; vi++)
            if (variants[vi].cheap_margin == scfg.cheap_margin) {
                SchedHint h = variants[vi];
                h.cheap_margin = 0.5 * scfg.cheap_margin;
                variants.push_back(h);
            }
        const size_t nv = variants.size();
        for (int w : {5, 10})
            for (size_t vi = 0; vi < nv; vi++) {
                SchedHint h = variants[vi];
                h.support_weight = w;
                variants.push_back(h);
            }
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
                sv.finish([&](Pass &&p) { cost += pass_time_cost(p, f32); });
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
        const size_t first_seeded = variants.size();
        constexpr int kSeeds = 16;
        // (the best three of each weight family, not of the whole list: the model ranks the families against each other only roughly)
        for (int w : {0, 5, 10}) {
            size_t taken = 0;
            for (size_t b = 0; b < order.size() && taken < 3; b++) {
                if (variants[order[b]].support_weight != w) continue;
                taken++;
                for (int sd = 1; sd <= kSeeds; sd++) {
                    SchedHint h = variants[order[b]];
                    h.seed = (uint64_t)sd;
                    variants.push_back(h);
                }
            }
        }
        evaluate(first_seeded, variants.size());
        reduce(first_seeded, variants.size());
    }
    return best;
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
    const uint64_t key = flush_rule(s, q, scfg.initial_support, false, true).key;
    if (key_out) *key_out = key;
    // A circuit whose schedule was chosen by measurement keeps it: no candidate is scheduled again (80 schedules cost about a
    // second at n = 30), and the hint is put back in case the hint table was emptied in between (kMaxSchedHints) — without
    // it the circuit would silently run its default schedule with the geometries measured for another one.
    RankedVariant kept{};
    if (measured_choice(key, kept)) {
        set_sched_hint(key, kept.hint, kept.is_default, scfg);
        if (ranked) ranked->clear(); // nothing left to try
        if (out) *out = schedule(with_hint(scfg, kept.hint), q);
        return;
    }
    // (Not on the cold path: the second buffer that out-of-place passes need cannot be asked for while the first is being allocated.)
    std::vector<SchedHint> variants;
    const size_t best = rank_schedules(scfg, q, s->f32, !stop && s->defer_flips != 0 && may_defer_flips(s), stop, variants, ranked);
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
    const std::vector<QueuedGate> q = queue_of(c);
    Scheduler sv(flush_rule(s, q, support, false).config(s)); // (a plain flush: a shard, whose flush may have a PackJob, never defers anyway)
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

namespace {
// A timed run on a stream: start(), the work, stop() — which waits for the stream to get there and reads the milliseconds in
// between.  Owns its two events on every return path.
class StreamTimer {
  public:
    explicit StreamTimer(hipStream_t stream) : stream_(stream) {}
    StreamTimer(const StreamTimer &) = delete;
    StreamTimer &operator=(const StreamTimer &) = delete;
    ~StreamTimer() {
        if (t0_) (void)hipEventDestroy(t0_);
        if (t1_) (void)hipEventDestroy(t1_);
    }
    int create() {
        HIP_TRY(hipEventCreate(&t0_));
        HIP_TRY(hipEventCreate(&t1_));
        return QSIM_OK;
    }
    void start() { (void)hipEventRecord(t0_, stream_); }
    int stop(const char *who, float &ms) { // who: "planning" or "tuning", in front of the failure's text
        (void)hipEventRecord(t1_, stream_);
        if (hipEventSynchronize(t1_) != hipSuccess) return fail(QSIM_ERR_DEVICE, "%s: event sync failed", who);
        if (hipEventElapsedTime(&ms, t0_, t1_) != hipSuccess) return fail(QSIM_ERR_DEVICE, "%s: event time failed", who);
        return QSIM_OK;
    }

  private:
    hipStream_t stream_;
    hipEvent_t t0_ = nullptr, t1_ = nullptr;
};
} // namespace

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
    // The same holds for the schedules packed with a support weight (SchedConfig::support_weight), with or without deferred X gates: the
    // model prices a pass by the coordinate cube it visits, so what they save shows only in part — a third family, its best always run.
    for (int family = 0; family < 3; family++) {
        size_t taken = 0;
        for (const RankedVariant &v : ranked) { // distinct predicted costs = (almost surely) distinct schedules
            if (family < 2 ? (v.hint.support_weight != 0 || v.hint.defer != family) : v.hint.support_weight == 0) continue;
            bool dup = false;
            for (const RankedVariant &t : tries) dup = dup || t.cost == v.cost;
            if (!dup) { tries.push_back(v); taken++; }
            if (taken == (size_t)s->tune_schedules) break;
        }
    }
    StreamTimer timer(s->stream);
    QSIM_TRY(timer.create());
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
            else { s->zero_ket_pending = false; s->partial = false; s->region_pending = false; } // a dense state: whatever the buffer holds
            if (rc) break;
            timer.start();
            rc = qsim_run_circuit(s, c, 0, -1);
            if (rc == QSIM_OK) rc = qsim_flush(s);
            if (rc == QSIM_OK) rc = timer.stop("planning", ms);
        }
        if (i == 0 || ms < best_ms) { best_ms = ms; best_i = i; }
    }
    s->profile = saved_profile;
    s->stats.gates -= std::min<uint64_t>(s->stats.gates, (uint64_t)c->count * 2 * tries.size()); // planning runs are not gate statements of the caller
    if (rc) return rc;
    set_sched_hint(sched_key, tries[best_i].hint, tries[best_i].is_default, scfg);
    remember_measured_choice(sched_key, tries[best_i]);
    passes = schedule(with_hint(scfg, tries[best_i].hint), queue_of(c)); // the schedule that won: its tile-bit orders are measured next
    return qsim_sync(s);
}

// Times every tile pass of `passes` whose geometry is not in the table yet under candidate orders of its high bits and enters
// the fastest (qsim_tune_circuit's comment).  The state's contents are scratch here; the buffers keep their roles.
// support: where the state can be non-zero when the first pass starts (0: a reset, ~0: dense).  A pass over a partial support is
// timed as it will run — on that support, its new bits topmost in every candidate — and entered under a key of its own.
static uint64_t high_mask(const TileGeom &g) {
    uint64_t m = 0;
    for (int j = 0; j < g.n_high; j++) m |= 1ULL << g.high[j];
    return m;
}
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
        if (tile_order_known(s, p.geom, zero_mask)) { r.already_known++; continue; }
        const uint64_t new_mask = zero_mask & high_mask(p.geom);
        bool dup = false;
        for (const Todo &q : todo) dup = dup || (high_mask(q.p->geom) == high_mask(p.geom) && q.new_mask == new_mask);
        if (!dup) todo.push_back({&p, zero_mask, new_mask});
    }
    StreamTimer timer(s->stream);
    QSIM_TRY(timer.create());
    const auto t_begin = std::chrono::steady_clock::now();
    auto elapsed_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    void *const home = s->amps;
    const bool tune_oop = !todo.empty() && spare_buffer(s) != nullptr;
    uint64_t zero_mask = 0;
    auto timed = [&](const Pass &p, const TileGeom &g, float &ms) -> int {
        timer.start();
        QSIM_TRY(launch_tile_pass(s, p, g, false, nullptr, tune_oop, zero_mask)); // timed the way most passes of a run go
        return timer.stop("tuning", ms);
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
        TileGeom best = asc;
        const float ms_ascending = ms;
        float best_ms = ms;
        for (int cand = 1; cand < max_candidates; cand++) {
            if (cand >= 4 && elapsed_ms() > share_end) break;
            TileGeom g = asc;
            std::sort(g.high, g.high + g.n_high);
            shuffle_high(g, high_mask(asc) * 0x9E3779B97F4A7C15ULL + (uint64_t)cand * 0xD1B54A32D192ED03ULL);
            place_new_bits(g, todo[i].new_mask);
            rc = timed(p, g, ms);
            if (rc) break;
            r.candidates_timed++;
            if (ms < best_ms) { best_ms = ms; best = g; }
        }
        if (rc) break;
        if (best_ms < ms_ascending * 0.985f) { // keep ascending unless the gain is beyond the timing noise
            r.passes_reordered++;
        } else {
            best = asc;
            best_ms = ms_ascending;
        }
        r.ms_ascending += ms_ascending;
        r.ms_best += best_ms;
        r.passes_tuned++;
        enter_tile_order(s, best, todo[i].new_mask, best_ms, ms_ascending);
    }
    (void)hipStreamSynchronize(s->stream);
    if (s->amps != home) std::swap(s->amps, s->spare); // contents are scratch here (reset below); the buffers keep their roles
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
