// pass_builder.cpp — the scheduler's second half (scheduler.h): closed clusters into passes.  single_op_pass and tile_pass emit
// a pass; at level 3 build_passes groups the clusters into tile passes with PassBuilder's steps, all of which look at the pending
// clusters through the ONE PendingWalk.  Pure host code.
#include "scheduler_impl.h"

namespace qsim {

using sched::is_one;
using sched::to_block;

void Scheduler::single_op_pass(const FusedOp &op, const PassSink &sink) const {
    const double S = 16.0 * (double)(1ULL << cfg_.n); // bytes of state
    Pass p;
    p.src = cur_src_;
    p.ops.push_back(op);
    if (op.kind == OP_G1) {
        if (op.is_identity()) return;
        if (op.is_diag()) {
            p.kclass = QSIM_K_PHASE;
            const bool unit0 = is_one(op.m[0]);
            p.diag_full = !unit0 || op.q_hi < 2; // below 64-B runs every sector is touched anyway
            p.bytes = unit0 ? S : 2 * S;
        } else {
            p.kclass = op.q_hi >= 6 ? QSIM_K_GATE1 : QSIM_K_GATE1_LO;
            p.bytes = 2 * S;
        }
        sink(std::move(p));
    } else if (op.kind == OP_CX) {
        p.kclass = QSIM_K_CX;
        p.bytes = S;
        sink(std::move(p));
    } else {
        if (op.is_identity()) return;
        // a pair cluster that is still exactly one CX (nothing else was folded into it) moves half the state, not all
        // of it: the swap kernel instead of the dense 4x4 (or a tile pass)
        for (int hi_ctl = 0; hi_ctl < 2; hi_ctl++) {
            cd ref[16];
            cx4(hi_ctl != 0, ref);
            bool same = true;
            for (int k = 0; k < 16 && same; k++) same = op.m[k] == ref[k];
            if (!same) continue;
            FusedOp cx;
            cx.kind = OP_CX;
            cx.q_hi = hi_ctl ? op.q_hi : op.q_lo; // control
            cx.q_lo = hi_ctl ? op.q_lo : op.q_hi; // target
            cx.gates = op.gates;
            p.ops[0] = cx;
            p.kclass = QSIM_K_CX;
            p.bytes = S;
            sink(std::move(p));
            return;
        }
        if (op.kind == OP_G2 && op.q_lo >= 6) {
            p.kclass = QSIM_K_GATE2;
            p.bytes = 2 * S;
            sink(std::move(p));
        } else {
            tile_pass(p.ops, op.qmask(), sink);
        }
    }
}

uint64_t Scheduler::tile_pass(const std::vector<FusedOp> &ops, uint64_t hset, const PassSink &sink, uint64_t prefer) const {
    const int B = tile_.B, L = tile_.L;
    const uint64_t lowmask = tile_.lowmask;
    Pass p;
    p.src = cur_src_;
    p.kclass = QSIM_K_TILE;
    p.bytes = 32.0 * (double)(1ULL << cfg_.n);
    // `hset`: the high qubits the blocks NEED in the tile.  Qubits a block is merely block-diagonal in may stay outside
    // (they select a sub-block per tile); while slots are free they are taken in anyway, most used first, because a
    // block that lies entirely inside the tile can be merged with its neighbours.
    uint64_t high = hset & ~lowmask;
    {
        int uses[64] = {0};
        for (const FusedOp &op : ops)
            for (uint64_t rest = op.qmask() & ~lowmask & ~high; rest; rest &= rest - 1) uses[__builtin_ctzll(rest)]++;
        while (__builtin_popcountll(high) < B - L) {
            int best = -1;
            for (int b = L; b < cfg_.n; b++)
                if (uses[b] > 0 && (prefer >> b & 1ULL) && (best < 0 || uses[b] > uses[best])) best = b;
            if (best < 0) break;
            high |= 1ULL << best;
            uses[best] = 0;
        }
    }
    // unused slots are filled with free bits starting at pad_from, wrapping around to the low end.  Measured at
    // n = 30 (tools/pad_sweep.py): with three or four genuinely high qubits in the tile, padding with the lowest
    // bits (longest contiguous runs) costs up to 8.6 ms per pass against 6.8 ms when bits 10.. are used; 10 had the
    // best worst case over the geometries tried (<= 6.9 ms)
    const int start = cfg_.pad_from >= L && cfg_.pad_from < cfg_.n ? cfg_.pad_from : L;
    for (int round = 0; round < 2; round++) { // bits of `prefer` first: padding must not grow a partial state's support
        const uint64_t ok = round == 0 ? prefer : ~0ULL;
        for (int b = start; b < cfg_.n && __builtin_popcountll(high) < B - L; b++) if (ok >> b & 1ULL) high |= 1ULL << b;
        for (int b = L; b < start && __builtin_popcountll(high) < B - L; b++) if (ok >> b & 1ULL) high |= 1ULL << b;
    }
    p.geom.tile_bits = L + __builtin_popcountll(high);
    p.geom.low_bits = L;
    p.geom.n = cfg_.n;
    p.geom.n_high = 0;
    for (int b = L; b < cfg_.n; b++)
        if (high >> b & 1ULL) p.geom.high[p.geom.n_high++] = b;

    // Every block is split into the qubits it has inside the tile and the ones outside (it is block-diagonal in those:
    // build_passes only leaves such qubits out).  Blocks with nothing inside are tile-uniform factors: they commute
    // with everything else in the pass and go to the front, one entry per qubit set.
    const uint64_t tmask = lowmask | high;
    std::vector<TileBlock> scalars, blocks;
    for (const FusedOp &op : ops) {
        TileBlock tb = to_block(op, tmask);
        if (tb.nq > 0) { blocks.push_back(tb); continue; }
        bool folded = false;
        for (TileBlock &sc : scalars)
            if (sc.ns == tb.ns && sc.s[0] == tb.s[0] && sc.s[1] == tb.s[1]) {
                for (int v = 0; v < tb.banks(); v++) { // 1x1 banks: the factors multiply
                    const cd z = tb.at(v, 0, 0) * sc.at(v, 0, 0);
                    sc.row(v, 0).n = 1; sc.row(v, 0).col[0] = 0; sc.row(v, 0).val[0] = z;
                }
                sc.gates += tb.gates;
                folded = true;
                break;
            }
        if (!folded) scalars.push_back(tb);
    }
    if (cfg_.merge && blocks.size() > 1) merge_blocks(blocks);
    else blocks.erase(std::remove_if(blocks.begin(), blocks.end(), [](const TileBlock &t) { return t.is_identity(); }), blocks.end());
    scalars.erase(std::remove_if(scalars.begin(), scalars.end(), [](const TileBlock &t) { return t.is_identity(); }), scalars.end());
    p.geom.n_scale = (int)scalars.size();
    p.blocks = std::move(scalars);
    p.blocks.insert(p.blocks.end(), blocks.begin(), blocks.end());
    if (p.blocks.empty()) return 0; // every block was the identity: nothing is launched, nothing changes
    if (prefer != ~0ULL) { // the state's support is known: the pass visits the tiles inside support | tile
        const uint64_t all = index_mask(cfg_.n);
        p.visited = 1.0 / (double)(1ULL << (cfg_.n - __builtin_popcountll((prefer | tmask) & all)));
        // ... and reads the slots of those tiles that are inside the support already; nothing at all while there is no support (the
        // pass then generates the basis state)
        p.read_share = (prefer & all) == 0 ? 0.0 : p.visited / (double)(1ULL << __builtin_popcountll(tmask & ~prefer & all));
    }
    sink(std::move(p));
    return tmask;
}


// ---- level 3: clusters into tile passes ----------------------------------------------------------------------------------
namespace {

// What the walks know about the closed clusters: all qubits of each (ordering) and the ones that have to be tile qubits.
struct Clusters {
    std::vector<uint64_t> qm, must;
    bool commute = false;
    uint64_t all = 0;
};

// The ONE walk over the pending clusters of [from, to), in index order.  It owns the blocked qubits: `bm`, mixed by the pending
// clusters passed over so far, and `bs`, merely selecting in them.  A cluster is runnable when no earlier pending cluster
// blocks it, directly or through a chain of pending clusters, so clusters may be emitted in the order they are taken.
// Order: a cluster may run before an earlier pending one unless one of them MIXES a qubit they share — two clusters that
// are both block-diagonal in every shared qubit (controls of CXs, diagonal gates) commute.  (The first version chained
// everything on a shared qubit; with ~a quarter of the gates being CXs the controls were most of the chain.)
class PendingWalk { // plain pointers and values: the trial fills spend their time here, and the marks are written while it runs
  public:
    PendingWalk(const Clusters &cl, const std::vector<char> &done, size_t from, size_t to)
        : qm_(cl.qm.data()), must_(cl.must.data()), done_(done.data()), all_(cl.all), commute_(cl.commute), from_(from), to_(to), i_(from) {}
    // the next pending cluster, or -1: the range is at its end, or every qubit is blocked and nothing further can run (a branch of
    // its own, not folded into the cursor: the cursor must not wait for the blocked qubits)
    long next() {
        if (bm_ == all_) return -1;
        while (i_ < to_ && done_[i_]) i_++;
        return i_ < to_ ? (long)i_ : -1;
    }
    bool runnable(long i) const {
        if (!commute_) return (qm_[i] & (bm_ | bs_)) == 0;
        return (must_[i] & (bm_ | bs_)) == 0 && (qm_[i] & ~must_[i] & bm_) == 0;
    }
    uint64_t must(long i) const { return must_[i]; } // the qubits cluster i mixes
    void take(long i) { i_ = (size_t)i + 1; } // it runs: nothing is charged to the blocked qubits
    void pass_over(long i) {                  // it stays pending: its qubits are blocked for everything behind it
        bm_ |= must_[i];
        bs_ |= qm_[i] & ~must_[i];
        i_ = (size_t)i + 1;
    }
    void restart() { i_ = from_; bm_ = bs_ = 0; }

  private:
    const uint64_t *const qm_, *const must_;
    const char *const done_;
    const uint64_t all_;
    const bool commute_;
    const size_t from_, to_;
    size_t i_;
    uint64_t bm_ = 0, bs_ = 0;
};

struct Cand { long idx; int need; int rank; }; // rank: need, plus SchedConfig::support_weight per slot that would grow the support

} // namespace

// The state build_passes works on and its steps, in the order the loop at the end calls them.
class __attribute__((visibility("hidden"))) Scheduler::PassBuilder {
  public:
    PassBuilder(Scheduler &s, const PassSink &sink);
    void run();

  private:
    Scheduler &s_;
    const SchedConfig &cfg_;
    const TileShape &tile_;
    const PassSink &sink_;
    const size_t m_;
    Clusters cl_;
    std::vector<char> done_, trial_, work_;
    uint64_t rng_;  // xorshift64*: SchedConfig::seed
    int cap_;       // clusters per pass; lifted to tail_max_ops when that lets a pass finish the circuit
    size_t first_ = 0, end_ = 0; // the first pending cluster; the end of the window scanned from it
    bool endgame_ = false;       // few blocks left: search the last pass sets so that no straggler pass remains
    uint64_t support_;           // the state's support as the engine will track it (SchedConfig::initial_support): tile passes add their
                                 // tile's qubits, anything else makes the engine write the zeros out (dense from then on)
    std::vector<Cand> cands_;
    std::vector<long> picks_, best_picks_;
    std::vector<FusedOp> group_;

    uint64_t high_of(long i) const { return cl_.must[(size_t)i] & ~tile_.lowmask; } // the slots cluster i needs
    // SchedConfig::support_weight, while it counts: the support is neither empty (the generating pass reads nothing) nor complete
    int grow_weight() const { return cfg_.support_weight > 0 && support_ != 0 && support_ != cl_.all ? cfg_.support_weight : 0; }
    bool coin();
    size_t pending_from_first(size_t limit) const;
    void note(const std::vector<long> &idx);
    Cand scan(const std::vector<char> &dn, uint64_t hset, std::vector<Cand> *cands) const;
    // kept out of line: inlined into the rollouts its loop spills what it holds in registers here (4 % of the scheduler's host time)
    __attribute__((noinline)) int fill(std::vector<char> &dn, uint64_t &hset, int limit, uint64_t admit = ~0ULL) const;
    int rollout(std::vector<char> &dn, uint64_t hset, int have) const;
    int eval(const std::vector<char> &dn, uint64_t S, std::vector<long> *out, uint64_t *one_short = nullptr) const;
    int passes_to_finish(std::vector<char> &dn, int limit) const;
    int eval_ahead(uint64_t S, std::vector<long> *out, uint64_t *one_short = nullptr);

    bool pass_inside_support();
    void choose_cap();
    uint64_t grow_greedy();
    uint64_t swap_search(uint64_t hset);
    void emit(uint64_t hset);
};

Scheduler::PassBuilder::PassBuilder(Scheduler &s, const PassSink &sink)
    : s_(s), cfg_(s.cfg_), tile_(s.tile_), sink_(sink), m_(s.closed_.size()), done_(m_, 0),
      rng_(cfg_.seed * 0x9E3779B97F4A7C15ULL + 0xD1B54A32D192ED03ULL), cap_(cfg_.tile_max_ops) {
    cl_.commute = cfg_.selectors && cfg_.commute;
    cl_.all = index_mask(cfg_.n);
    cl_.qm.resize(m_);
    cl_.must.resize(m_);
    for (size_t i = 0; i < m_; i++) {
        cl_.qm[i] = s.closed_[i].qmask();
        cl_.must[i] = cfg_.selectors ? (cl_.qm[i] & ~s.closed_[i].selector_mask()) : cl_.qm[i];
    }
    support_ = cfg_.initial_support & cl_.all;
}

bool Scheduler::PassBuilder::coin() {
    if (!cfg_.seed) return false;
    rng_ ^= rng_ >> 12; rng_ ^= rng_ << 25; rng_ ^= rng_ >> 27;
    return ((rng_ * 0x2545F4914F6CDD1DULL) >> 63) != 0;
}

// pending clusters from first_, counted up to `limit` (one more means "more than that")
size_t Scheduler::PassBuilder::pending_from_first(size_t limit) const {
    size_t left = 0;
    for (size_t i = first_; i < m_ && left <= limit; i++) left += !done_[i];
    return left;
}

void Scheduler::PassBuilder::note(const std::vector<long> &idx) { // the gates behind the clusters of the pass about to be emitted
    s_.cur_src_.clear();
    if (!cfg_.track) return;
    for (long i : idx) s_.cur_src_.insert(s_.cur_src_.end(), s_.closed_src_[(size_t)i].begin(), s_.closed_src_[(size_t)i].end());
}

// Runnable blocks under the qubits chosen so far, cheapest (fewest new high-qubit slots) first.  While the support is partial a
// slot outside it costs support_weight more than its place in the tile: it doubles what this pass and every later one visits.
Cand Scheduler::PassBuilder::scan(const std::vector<char> &dn, uint64_t hset, std::vector<Cand> *cands) const {
    Cand best{-1, 1 << 30, 1 << 30};
    const int used = __builtin_popcountll(hset);
    const int gw = grow_weight();
    PendingWalk w(cl_, dn, first_, end_);
    for (long i; (i = w.next()) >= 0; w.pass_over(i)) {
        if (!w.runnable(i)) continue;
        const int need = __builtin_popcountll(high_of(i) & ~hset);
        if (used + need > tile_.kmax) continue;
        const int rank = gw ? need + gw * __builtin_popcountll(high_of(i) & ~hset & ~support_) : need;
        if (cands) cands->push_back({i, need, rank});
        if (rank < best.rank) {
            best = {i, need, rank};
            if (need == 0) return best; // free: take it right away
        }
    }
    return best;
}

// A pass filled greedily from (dn, hset): up to `limit` times the cluster scan() would return, marked done in dn and its
// qubits added to hset.  Same picks as calling scan() once per pick, without starting over each time: a pick that needs
// no new qubit (scan's early return) changes nothing for the clusters in front of it — the scan simply goes on behind
// it with the blocked qubits and the cheapest candidate seen so far; only a pick that admits a qubit (it comes after a
// whole scan) changes what the others need, and the next scan starts over.  (The local search fills ~4000 trial passes
// per schedule this way; with the pruned local search below 34 -> 15.6 ms of host time for the 1000 gates of the bench circuit.)
// (scan() without a support weight, that is: the trial fills and rollouts count what a pass can absorb, by slots alone.)
// `admit`: only clusters whose slots all lie in it are taken (the pass inside the support); the others are passed over.
int Scheduler::PassBuilder::fill(std::vector<char> &dn, uint64_t &hset, int limit, uint64_t admit) const {
    int cnt = 0;
    Cand best{-1, 1 << 30, 0};
    const uint64_t himask = ~tile_.lowmask;
    const int kmax = tile_.kmax;
    uint64_t h = hset;
    int used = __builtin_popcountll(h);
    PendingWalk w(cl_, dn, first_, end_);
    while (cnt < limit) {
        long free_pick = -1;
        for (long i; (i = w.next()) >= 0; w.pass_over(i)) {
            if (!w.runnable(i)) continue;
            const uint64_t high = w.must(i) & himask;
            if (high & ~admit) continue;
            const int need = __builtin_popcountll(high & ~h);
            if (need == 0) { free_pick = i; break; } // used + 0 <= kmax always holds
            if (used + need <= kmax && need < best.need) best = {i, need, 0};
        }
        if (free_pick >= 0) {
            dn[(size_t)free_pick] = 1;
            cnt++;
            w.take(free_pick);
            continue;
        }
        if (best.idx < 0) break;
        dn[(size_t)best.idx] = 1;
        h |= high_of(best.idx);
        cnt++;
        w.restart();
        best = {-1, 1 << 30, 0};
        used = __builtin_popcountll(h);
    }
    hset = h;
    return cnt;
}

// how many blocks a pass reaches when it is finished greedily from (dn, hset)
int Scheduler::PassBuilder::rollout(std::vector<char> &dn, uint64_t hset, int have) const {
    int cnt = fill(dn, hset, cap_ - have);
    // look further: what the following passes reach when each is simply built greedily
    for (int extra = 0; extra < cfg_.lookahead; extra++) {
        uint64_t h2 = 0;
        cnt += fill(dn, h2, cap_);
    }
    return cnt;
}

// Blocks a pass with high-qubit set S executes, in index order (a valid execution order: a block runs only if
// every earlier pending block on its qubits ran), and their score.
// one_short (optional): the qubits b for which some cluster the walk reaches could run if b alone were added to S.  For any
// other b, S | b executes exactly what S executes (the first cluster to be treated differently would have to be one of those).
int Scheduler::PassBuilder::eval(const std::vector<char> &dn, uint64_t S, std::vector<long> *out, uint64_t *one_short) const {
    int score = 0, cnt = 0;
    if (out) out->clear();
    PendingWalk w(cl_, dn, first_, end_);
    for (long i; cnt < cap_ && (i = w.next()) >= 0;) {
        const bool free_to_run = w.runnable(i);
        const uint64_t missing = high_of(i) & ~S;
        if (free_to_run && !missing) {
            score += cfg_.objective ? (int)s_.closed_[(size_t)i].gates : 1;
            cnt++;
            if (out) out->push_back(i);
            w.take(i);
        } else {
            if (one_short && free_to_run && !(missing & (missing - 1))) *one_short |= missing;
            w.pass_over(i);
        }
    }
    return score;
}

// greedy passes needed to finish everything pending in the window (at most `limit` are tried)
int Scheduler::PassBuilder::passes_to_finish(std::vector<char> &dn, int limit) const {
    int n_pass = 0;
    for (; n_pass < limit; n_pass++) {
        bool pending = false;
        for (size_t i = first_; i < end_ && !pending; i++) pending = !dn[i];
        if (!pending) break;
        uint64_t h2 = 0;
        if (fill(dn, h2, cap_) == 0) return limit; // cannot happen (a pass always takes something); keeps the loop finite
    }
    return n_pass;
}

int Scheduler::PassBuilder::eval_ahead(uint64_t S, std::vector<long> *out, uint64_t *one_short) {
    std::vector<long> &picks = out ? *out : picks_;
    int score = eval(done_, S, &picks, one_short);
    if (cfg_.lookahead > 0 || endgame_) {
        trial_ = done_;
        for (long i : picks) trial_[(size_t)i] = 1;
        if (endgame_) {
            // near the end what counts is how many MORE sweeps over the state the circuit needs (a straggler pass for
            // a handful of gates costs as much as a full one): fewer first, then more clusters in this pass
            const int more = passes_to_finish(trial_, 8);
            score += (8 - more) * 100000;
        } else {
            score += rollout(trial_, 0, 0); // the next pass, built greedily (plus cfg_.lookahead more inside)
        }
    }
    return score;
}

// Step 1, while the support is partial.  A pass that stays inside the support visits 2^(|support| - n) of the register: the
// greedy fill with the support as the only qubits admitted, kept when it absorbs more clusters than its share of a full sweep
// is worth.  true: the pass was emitted.
bool Scheduler::PassBuilder::pass_inside_support() {
    if (support_ == cl_.all || support_ == 0 || !(cfg_.cheap_margin > 0)) return false;
    work_ = done_;
    uint64_t h0 = 0;
    const int got = fill(work_, h0, cfg_.tile_max_ops, support_);
    const double share = 1.0 / (double)(1ULL << (cfg_.n - __builtin_popcountll(support_)));
    if (got < 2 || (double)got < cfg_.cheap_margin * (double)cfg_.tile_max_ops * share) return false;
    picks_.clear();
    for (size_t i = first_; i < end_; i++) // in index order, from the done-marks
        if (work_[i] && !done_[i]) picks_.push_back((long)i);
    for (long i : picks_) { group_.push_back(s_.closed_[(size_t)i]); done_[(size_t)i] = 1; }
    note(picks_);
    if (const uint64_t tmask = s_.tile_pass(group_, h0, sink_, support_)) support_ |= tmask;
    return true;
}

// Step 2.  The cap balances a pass's block phase against its memory time; a pass that would leave only a few clusters
// for one more sweep over the state (6.6 ms at n = 30 for, on the bench circuit, ONE gate) takes them instead.  The same
// count says whether the endgame has begun.
void Scheduler::PassBuilder::choose_cap() {
    const size_t tile_ops = (size_t)cfg_.tile_max_ops;
    const size_t left = pending_from_first(std::max((size_t)std::max(cfg_.tail_max_ops, cfg_.tile_max_ops), 2 * tile_ops));
    cap_ = (cfg_.tail_max_ops > cfg_.tile_max_ops && left <= (size_t)cfg_.tail_max_ops) ? cfg_.tail_max_ops : cfg_.tile_max_ops;
    endgame_ = left <= 2 * tile_ops;
}

// Step 3.  Greedy construction on a copy: cheapest new qubit first, ties broken by a rollout.  Returns the high-qubit set.
uint64_t Scheduler::PassBuilder::grow_greedy() {
    uint64_t hset = 0;
    work_ = done_;
    for (int have = 0; have < cap_; have++) {
        cands_.clear();
        Cand pick = scan(work_, hset, cfg_.rollout > 1 ? &cands_ : nullptr);
        if (pick.idx < 0) break;
        if (pick.need > 0 && cfg_.rollout > 1 && cands_.size() > 1) {
            // a new qubit has to be admitted: try the cheapest few candidates and keep the one after which a
            // greedy completion of this pass absorbs the most blocks
            std::stable_sort(cands_.begin(), cands_.end(), [](const Cand &a, const Cand &b) { return a.rank < b.rank; });
            int best_score = -1;
            const size_t tries = std::min(cands_.size(), (size_t)cfg_.rollout);
            for (size_t t = 0; t < tries; t++) {
                trial_ = work_;
                trial_[(size_t)cands_[t].idx] = 1;
                const int score = rollout(trial_, hset | high_of(cands_[t].idx), have + 1);
                if (score > best_score || (score == best_score && coin())) { best_score = score; pick = cands_[t]; }
            }
        }
        hset |= high_of(pick.idx);
        work_[(size_t)pick.idx] = 1;
    }
    return hset;
}

// Step 4.  Local search over the qubit set: swap one chosen high qubit for one left out while the pass (and, with
// lookahead, the greedy passes after it) executes more.  The host has milliseconds per pass to spend here:
// the GPU is busy with the previous pass for ~7 ms at n = 30.
uint64_t Scheduler::PassBuilder::swap_search(uint64_t hset) {
    const int iters = endgame_ ? std::max(cfg_.local_iters, 3) : cfg_.local_iters;
    if (iters <= 0 || __builtin_popcountll(hset) < 2) return hset;
    // ... less support_weight per chosen qubit outside the partial support (grow_weight): a set that absorbs a few clusters more
    // by doubling the visited share does not win
    const int gw = grow_weight();
    auto growth = [&](uint64_t S) { return gw ? gw * __builtin_popcountll(S & ~support_) : 0; };
    int best = eval_ahead(hset, &best_picks_) - growth(hset);
    for (int it = 0; it < iters; it++) {
        uint64_t bestS = hset;
        for (uint64_t in = hset; in; in &= in - 1) {
            const uint64_t qi = in & (0 - in);
            // the set without qi, once: most qubits b put in qi's place change nothing about what the pass executes
            // (no reachable cluster is short of exactly b), and those all score what the smaller set scores
            uint64_t one_short = 0;
            const int v_without = eval_ahead(hset & ~qi, nullptr, &one_short);
            for (int b = tile_.L; b < cfg_.n; b++) {
                if (hset >> b & 1ULL) continue;
                const uint64_t S2 = (hset & ~qi) | (1ULL << b);
                const int v = ((one_short >> b & 1ULL) ? eval_ahead(S2, nullptr) : v_without) - growth(S2);
                if (v > best || (v == best && bestS != hset && coin())) { best = v; bestS = S2; }
            }
        }
        if (bestS == hset) break;
        hset = bestS;
    }
    return hset;
}

// Step 5.  The clusters the chosen set executes become the pass.
void Scheduler::PassBuilder::emit(uint64_t hset) {
    eval(done_, hset, &best_picks_);
    if (best_picks_.empty()) { // the set cannot be worse than the greedy one; keep the scheduler total anyway
        best_picks_.push_back((long)first_);
        hset = high_of((long)first_);
    }
    for (long i : best_picks_) {
        group_.push_back(s_.closed_[(size_t)i]);
        done_[(size_t)i] = 1;
    }
    note(group_.empty() ? std::vector<long>{(long)first_} : best_picks_);
    if (group_.empty()) { // cannot happen while kmax >= 2; keep the scheduler total anyway
        s_.single_op_pass(s_.closed_[first_], sink_);
        done_[first_] = 1;
        support_ = cl_.all;
    } else if (group_.size() == 1) {
        s_.single_op_pass(group_[0], sink_); // may be a tile pass of its own or a single-gate kernel: count it as dense
        support_ = cl_.all;
    } else if (const uint64_t tmask = s_.tile_pass(group_, hset, sink_, support_ == cl_.all ? ~0ULL : support_)) {
        support_ |= tmask;
    }
}

void Scheduler::PassBuilder::run() {
    while (first_ < m_) {
        if (done_[first_]) { first_++; continue; }
        group_.clear();
        end_ = std::min(m_, first_ + (size_t)cfg_.window);
        if (pass_inside_support()) continue;
        choose_cap();
        emit(swap_search(grow_greedy()));
    }
}

void Scheduler::build_passes(const PassSink &sink) {
    if (cfg_.fuse <= 2) {
        for (size_t i = 0; i < closed_.size(); i++) {
            cur_src_.clear();
            if (cfg_.track) cur_src_ = closed_src_[i];
            single_op_pass(closed_[i], sink);
        }
        return;
    }
    PassBuilder(*this, sink).run();
}

} // namespace qsim
