// wisdom.cpp — everything the engine knows by MEASUREMENT or by having tried schedules, kept per process: the tile-bit orders
// measured per pass geometry ("wisdom"), the schedule hint per circuit and the schedule choices that were measured, with their
// file format (qsim_tune_table_*).
// The three tables, their two locks and the epoch are private to this file.  engine.cpp reaches them through order_tile_bits,
// apply_sched_hint, have_sched_hints and wisdom_epoch (engine_state.h), the planning step through the functions of planning.h.
// Pure host code: no HIP call, no device.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include "planning.h"

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
static std::atomic<uint64_t> g_wisdom_epoch{1}; // bumped whenever a table changes: cached plans carry the orders and the schedule they were built with

static GeomKey geom_key(const qsim_state *s, const TileGeom &g, uint64_t new_mask = 0) {
    GeomKey k{g.n, s->f32 ? 1 : 0, g.tile_bits, g.low_bits, 0, 0};
    for (int j = 0; j < g.n_high; j++) k.high_mask |= 1ULL << g.high[j];
    k.new_mask = new_mask & k.high_mask;
    return k;
}

void qsim::shuffle_high(TileGeom &g, uint64_t seed) {
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
        shuffle_high(g, probe_order_seed((uint64_t)s->debug_tile_order, s->tile_passes));
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

bool qsim::tile_order_known(const qsim_state *s, const TileGeom &g, uint64_t new_mask) {
    std::lock_guard<std::mutex> lock(g_wisdom_mu);
    return g_wisdom.count(geom_key(s, g, new_mask)) != 0;
}

void qsim::enter_tile_order(const qsim_state *s, const TileGeom &g, uint64_t new_mask, float ms, float ms_ascending) {
    GeomOrder o{};
    for (int j = 0; j < g.n_high; j++) o.high[j] = (int8_t)g.high[j];
    o.ms = ms;
    o.ms_ascending = ms_ascending;
    std::lock_guard<std::mutex> lock(g_wisdom_mu);
    g_wisdom[geom_key(s, g, new_mask)] = o;
    g_wisdom_epoch++;
}

// Scheduler variant per circuit, decided by the planning step (qsim_tune_circuit): key -> SchedConfig::commute and the other
// fields of SchedHint.  Circuits that were never planned use the default.
// The table is found by key alone: a colliding circuit would be scheduled with another circuit's variant — a valid schedule
// either way (every variant is; the results never depend on it).  Bounded: beyond kMaxSchedHints circuits it starts afresh.
static std::mutex g_hints_mu;
static std::map<uint64_t, SchedHint> g_sched_hints;
constexpr size_t kMaxSchedHints = 4096;
// circuits whose schedule was chosen by MEASUREMENT (qsim_tune_circuit): the choice stands until the table is cleared — timing
// the same candidates again could flip between near-equal schedules and invalidate the geometries measured for the winner
static std::map<uint64_t, RankedVariant> g_sched_measured; // guarded by g_hints_mu

SchedConfig qsim::with_hint(SchedConfig v, const SchedHint &h) {
    v.commute = h.commute; v.cheap_margin = h.cheap_margin; v.lookahead = h.lookahead; v.seed = h.seed; v.defer_flips = h.defer;
    v.support_weight = h.support_weight;
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

// How the hint table states a choice (the caller holds g_hints_mu): the default schedule is the ABSENCE of a hint.
// rescheduled: cached plans of this circuit were scheduled another way, so they must not be replayed.
static void put_hint(uint64_t key, const SchedHint &h, bool is_default, bool rescheduled) {
    if (is_default) g_sched_hints.erase(key);
    else g_sched_hints[key] = h;
    if (rescheduled) g_wisdom_epoch++;
}

void qsim::set_sched_hint(uint64_t key, const SchedHint &now, bool is_default, const SchedConfig &scfg) {
    std::lock_guard<std::mutex> lock(g_hints_mu);
    const auto it = g_sched_hints.find(key);
    const SchedHint dflt{scfg.commute, scfg.cheap_margin, scfg.lookahead, 0, 0, 0, scfg.support_weight};
    const SchedHint before = it == g_sched_hints.end() ? dflt : it->second;
    if (!is_default && g_sched_hints.size() >= kMaxSchedHints && it == g_sched_hints.end()) { // full: both tables start over together — a
        g_sched_hints.clear();                                              // measured entry without its hint would pin a schedule nobody runs
        const auto mine = g_sched_measured.find(key);
        const bool keep = mine != g_sched_measured.end();
        const RankedVariant kept = keep ? mine->second : RankedVariant{};
        g_sched_measured.clear();
        if (keep) g_sched_measured[key] = kept;
    }
    put_hint(key, now, is_default, before.commute != now.commute || before.cheap_margin != now.cheap_margin || before.lookahead != now.lookahead ||
                                       before.cap != now.cap || before.seed != now.seed || before.defer != now.defer ||
                                       before.support_weight != now.support_weight);
}

bool qsim::measured_choice(uint64_t key, RankedVariant &out) {
    std::lock_guard<std::mutex> lock(g_hints_mu);
    const auto it = g_sched_measured.find(key);
    if (it == g_sched_measured.end()) return false;
    out = it->second;
    return true;
}

void qsim::remember_measured_choice(uint64_t key, const RankedVariant &choice) {
    std::lock_guard<std::mutex> lock(g_hints_mu);
    if (g_sched_measured.size() >= kMaxSchedHints) g_sched_measured.clear();
    g_sched_measured[key] = choice;
}

// The measured schedule choice filed under a key (what a "sched" line of the file holds): 1 and the setting, or 0.
extern "C" int qsim_sched_choice_lookup(uint64_t key, qsim_sched_setting *out) {
    RankedVariant rv{};
    if (!out || !measured_choice(key, rv)) return 0;
    *out = qsim_sched_setting{};
    out->commute = rv.hint.commute; out->lookahead = rv.hint.lookahead; out->cap = rv.hint.cap; out->defer = rv.hint.defer;
    out->support_weight = rv.hint.support_weight; out->is_default = rv.is_default ? 1 : 0; out->seed = rv.hint.seed; out->cheap_margin = rv.hint.cheap_margin;
    return 1;
}
// ... and a choice filed as if it had been measured (the planning step does this on a device; tests of the file format do it here)
extern "C" int qsim_sched_choice_enter(uint64_t key, const qsim_sched_setting *in) {
    if (!in || !(in->cheap_margin > 0) || in->lookahead < 0 || in->commute < 0 || in->cap < 0 || in->support_weight < 0) return fail(QSIM_ERR_ARG, "scheduler setting out of range");
    RankedVariant rv{};
    rv.hint = {in->commute, in->cheap_margin, in->lookahead, in->cap, in->seed, in->defer != 0 ? 1 : 0, in->support_weight};
    rv.is_default = in->is_default != 0;
    remember_measured_choice(key, rv);
    return QSIM_OK;
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
    {   // measured schedule choices: "sched <key> <commute> <cheap_margin> <lookahead> <cap> <is_default> <seed> [<defer> [<support_weight>]]"
        std::lock_guard<std::mutex> lock(g_hints_mu);
        for (const auto &kv : g_sched_measured) {
            fprintf(f, "sched %llx %d %.17g %d %d %d %llu", (unsigned long long)kv.first, kv.second.hint.commute, kv.second.hint.cheap_margin,
                    kv.second.hint.lookahead, kv.second.hint.cap, kv.second.is_default ? 1 : 0, (unsigned long long)kv.second.hint.seed);
            // an eighth field only where X gates are deferred, a ninth (SchedConfig::support_weight, the eighth then always in front of
            // it) only where the weight is not 0: other lines stay what older files hold
            if (kv.second.hint.support_weight) fprintf(f, " %d %d", kv.second.hint.defer ? 1 : 0, kv.second.hint.support_weight);
            else if (kv.second.hint.defer) fprintf(f, " 1");
            fprintf(f, "\n");
        }
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
            if (sscanf(line + 6, "%llx %d %lf %d %d %d %llu %d %d", &key, &rv.hint.commute, &rv.hint.cheap_margin, &rv.hint.lookahead, &rv.hint.cap, &isd, &seed, &rv.hint.defer,
                       &rv.hint.support_weight) >= 6 && // (fewer than nine fields: an older line, weight 0)
                (rv.hint.defer == 0 || rv.hint.defer == 1) && rv.hint.support_weight >= 0 && rv.hint.support_weight <= 1024 &&
                rv.hint.cheap_margin > 0 && rv.hint.lookahead >= 0 && rv.hint.lookahead <= 8 && rv.hint.cap >= 0 && rv.hint.cap <= 512) {
                rv.is_default = isd != 0;
                rv.hint.seed = seed;
                std::lock_guard<std::mutex> lock(g_hints_mu);
                g_sched_measured[key] = rv;
                put_hint(key, rv.hint, rv.is_default, true);
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
