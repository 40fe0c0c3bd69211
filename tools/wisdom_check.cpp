// wisdom_check.cpp — a stand-alone check of csrc/wisdom.cpp (the process-wide planning tables and their file format) under the host
// sanitizers.  wisdom.cpp makes no HIP call, so this program opens no device: it supplies qsim::fail itself and builds qsim_state
// values on the host.  From the repository root:
//   hipcc -std=c++17 -O1 -g -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/wisdom_check.cpp gpu_quantum_simulator_amd/csrc/wisdom.cpp -o wisdom_check && ./wisdom_check DIR
// It writes three small files into DIR, prints the number of checks and exits 1 at the first that fails.
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../gpu_quantum_simulator_amd/csrc/planning.h"

using namespace qsim;

int qsim::fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}

static int g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        g_checks++;                                                          \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static TileGeom geom(int n, int tile_bits, int low_bits, std::vector<int> high) {
    TileGeom g{};
    g.n = n; g.tile_bits = tile_bits; g.low_bits = low_bits; g.n_high = (int)high.size();
    for (size_t j = 0; j < high.size(); j++) g.high[j] = high[j];
    return g;
}
static std::vector<int> order(const TileGeom &g) { return std::vector<int>(g.high, g.high + g.n_high); }
static std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    const std::string in = dir + "/wisdom_in.txt", a = dir + "/wisdom_a.txt", b = dir + "/wisdom_b.txt";
    {   // five lines the loader takes, then one of every kind it rejects
        std::ofstream f(in);
        f << "20 0 8 3 f8 1.5000 2.0000 7 3 5 4 6\n"                   // a full pass
          << "part c0 20 0 8 3 f8 1.0000 1.2500 4 3 5 7 6\n"          // the same set with bits 6 and 7 new: they are topmost
          << "sched abc 1 0.5 1 0 1\n"                                // 6 fields (files from before the seed)
          << "sched abd 0 0.25 2 24 0 5\n"                            // 7 fields
          << "sched abe 1 0.5 0 28 0 3 1\n"                           // 8 fields: X gates deferred
          << "part 0 20 0 8 3 f8 1.0 1.0 3 4 5 6 7\n"                 // part without new bits
          << "part zz 20 0 8 3 f8 1.0 1.0 3 4 5 6 7\n"                // part without a mask
          << "part 100 20 0 8 3 f8 1.0 1.0 3 4 5 6 7\n"               // new bits outside the set
          << "part c0 20 0 8 3 f8 1.0 1.0 6 7 3 4 5\n"                // new bits not topmost
          << "20 0 8 3 f8 1.0\n"                                      // too few fields
          << "20 0 8 3 8 1.0 1.0 3\n"                                 // fewer than two high bits
          << "20 0 14 3 3ff8 1.0 1.0 3 4 5 6 7 8 9 10 11 12 13\n"     // more than kMaxTileHigh
          << "20 0 8 3 f8 1.0 1.0 3 4 5 6\n"                          // order too short
          << "20 0 8 3 f8 1.0 1.0 3 4 5 6 6\n"                        // a bit twice
          << "20 0 8 3 f8 1.0 1.0 3 4 5 6 9\n"                        // a bit outside the set
          << "20 0 8 3 f8 1.0 1.0 3 4 5 6 99\n"                       // no bit at all
          << "garbage\n"
          << "sched abf 1 0.5 1 0\n"                                  // too few fields
          << "sched abf 1 0.5 1 0 0 0 2\n"                            // defer not 0 / 1
          << "sched abf 1 0 1 0 0\n"                                  // cheap_margin not positive
          << "sched abf 1 0.5 9 0 0\n"                                // lookahead out of range
          << "sched abf 1 0.5 1 513 0\n";                             // cap out of range
    }
    uint64_t epoch = wisdom_epoch();
    CHECK(qsim_tune_table_load(in.c_str()) == 5);
    CHECK(qsim_tune_table_size() == 2);
    CHECK(wisdom_epoch() == epoch + 5); // every line taken bumps it
    CHECK(qsim_tune_table_load((dir + "/no_such_file").c_str()) == -1 && qsim_tune_table_load(nullptr) == -1);
    RankedVariant rv{};
    CHECK(measured_choice(0xabc, rv) && rv.is_default && rv.hint.commute == 1 && rv.hint.seed == 0 && rv.hint.defer == 0);
    CHECK(measured_choice(0xabd, rv) && !rv.is_default && rv.hint.cap == 24 && rv.hint.seed == 5 && rv.hint.cheap_margin == 0.25);
    CHECK(measured_choice(0xabe, rv) && rv.hint.defer == 1 && rv.hint.seed == 3);
    CHECK(!measured_choice(0xabf, rv));
    SchedConfig base{}, cfg = base;
    apply_sched_hint(0xabc, cfg); // a default choice is no hint
    CHECK(cfg.commute == base.commute && cfg.cheap_margin == base.cheap_margin && cfg.tile_max_ops == base.tile_max_ops);
    apply_sched_hint(0xabd, cfg);
    CHECK(cfg.commute == 0 && cfg.cheap_margin == 0.25 && cfg.lookahead == 2 && cfg.tile_max_ops == 24 && cfg.seed == 5 && cfg.defer_flips == 0);

    // save, load again, save again: the two files are equal
    CHECK(qsim_tune_table_save(a.c_str()) == QSIM_OK);
    qsim_tune_table_clear();
    CHECK(qsim_tune_table_size() == 0 && !have_sched_hints() && !measured_choice(0xabd, rv));
    CHECK(qsim_tune_table_load(a.c_str()) == 5);
    CHECK(qsim_tune_table_save(b.c_str()) == QSIM_OK);
    CHECK(!slurp(a).empty() && slurp(a) == slurp(b));

    // order_tile_bits: a known and an unknown key, with and without bits new to the support
    qsim_state s;
    s.n = 20;
    TileGeom g = geom(20, 8, 3, {3, 4, 5, 6, 7});
    order_tile_bits(&s, g);
    CHECK(s.tile_passes == 1 && order(g) == (std::vector<int>{7, 3, 5, 4, 6}));
    g = geom(20, 8, 3, {3, 4, 5, 6, 7});
    order_tile_bits(&s, g, 0xc0 | 1ULL << 15); // bits outside the tile do not count
    CHECK(order(g) == (std::vector<int>{4, 3, 5, 7, 6}));
    g = geom(20, 8, 3, {12, 11, 10, 9, 8});
    order_tile_bits(&s, g);
    CHECK(order(g) == (std::vector<int>{12, 11, 10, 9, 8})); // nothing measured: the order it came in
    const uint64_t zero_mask = 1ULL << 11 | 1ULL << 9 | 1ULL << 2;
    std::vector<int> want;
    for (int pass = 0; pass < 2; pass++) // the bits the state is not zero in first, the new ones topmost, each group in its order
        for (int bit : {12, 11, 10, 9, 8})
            if ((int)(zero_mask >> bit & 1) == pass) want.push_back(bit);
    order_tile_bits(&s, g, zero_mask);
    CHECK(order(g) == want && want == (std::vector<int>{12, 10, 8, 11, 9}));
    s.f32 = true; // another key: precision is part of it
    g = geom(20, 8, 3, {3, 4, 5, 6, 7});
    order_tile_bits(&s, g);
    CHECK(order(g) == (std::vector<int>{3, 4, 5, 6, 7}));
    epoch = wisdom_epoch();
    CHECK(!tile_order_known(&s, g, 0));
    enter_tile_order(&s, geom(20, 8, 3, {6, 5, 7, 4, 3}), 0, 1.f, 2.f);
    CHECK(tile_order_known(&s, g, 0) && !tile_order_known(&s, g, 0x80) && wisdom_epoch() == epoch + 1 && qsim_tune_table_size() == 3);
    order_tile_bits(&s, g);
    CHECK(order(g) == (std::vector<int>{6, 5, 7, 4, 3}));
    g = geom(20, 4, 3, {9});
    order_tile_bits(&s, g, 1ULL << 9);
    CHECK(s.tile_passes == 7 && order(g) == (std::vector<int>{9})); // a single high bit: counted, not ordered

    // the probe orders of QSIM_OPT_DEBUG_TILE_ORDER: shuffle_high under probe_order_seed(k, pass count), the table not consulted
    for (int k = 1; k <= 2; k++) {
        s.debug_tile_order = k;
        g = geom(20, 8, 3, {3, 4, 5, 6, 7});
        TileGeom ref = g;
        const uint64_t pass = s.tile_passes + 1;
        CHECK(probe_order_seed((uint64_t)k, pass) == 0x9E3779B97F4A7C15ULL * (uint64_t)(k + 1) + 0xD1B54A32D192ED03ULL * pass);
        shuffle_high(ref, probe_order_seed((uint64_t)k, pass));
        order_tile_bits(&s, g, 0xc0);
        CHECK(s.tile_passes == pass && order(g) == order(ref) && order(g) != (std::vector<int>{6, 5, 7, 4, 3}));
        std::vector<int> sorted = order(g);
        std::sort(sorted.begin(), sorted.end());
        CHECK(sorted == (std::vector<int>{3, 4, 5, 6, 7}));
    }

    // the hint table is bounded (kMaxSchedHints = 4096): the set that finds it full restarts both tables together and keeps its own
    // measured entry
    qsim_tune_table_clear();
    const SchedHint hint{0, 0.75, 1, 24, 9, 0};
    const uint64_t mine = 0x5555555555ULL, other = 0x7777777777ULL;
    for (uint64_t key = 1; key <= 4096; key++) set_sched_hint(key, hint, false, base);
    remember_measured_choice(mine, RankedVariant{hint, 3.5, false});
    remember_measured_choice(other, RankedVariant{hint, 4.5, false});
    epoch = wisdom_epoch();
    set_sched_hint(1, hint, false, base); // a key the table has, set to what it has: nothing happens
    CHECK(wisdom_epoch() == epoch && measured_choice(other, rv));
    set_sched_hint(mine, hint, false, base);
    CHECK(wisdom_epoch() == epoch + 1);
    CHECK(measured_choice(mine, rv) && rv.cost == 3.5 && rv.hint.cap == 24 && !measured_choice(other, rv));
    cfg = base;
    apply_sched_hint(1, cfg);
    CHECK(have_sched_hints() && cfg.cheap_margin == base.cheap_margin && cfg.seed == base.seed);
    apply_sched_hint(mine, cfg);
    CHECK(cfg.cheap_margin == 0.75 && cfg.seed == 9 && cfg.tile_max_ops == 24 && cfg.tail_max_ops >= 24);
    set_sched_hint(mine, SchedHint{base.commute, base.cheap_margin, base.lookahead, 0, 0, 0}, true, base); // the default is the absence of a hint
    CHECK(!have_sched_hints() && wisdom_epoch() == epoch + 2 && measured_choice(mine, rv));
    qsim_tune_table_clear();
    printf("wisdom_check: %d checks passed\n", g_checks);
    return 0;
}
