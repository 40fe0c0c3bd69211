// scheduler.h — host-side gate scheduler (no device code): turns the queued gate stream into passes.
//
// Reference rows: a10 fusion algebra (quantum_simulator_4x4.cu:148-250: mm2x2, mm4x4,
// tensorProd, cnotTo4x4), a11 pair state machine (quantum_simulator_4x4.cu:327-501; 2x2-only form
// quantum_simulator_preproces.cu:215-269), a12 op list for a single launch
// (quantum_simulator_preproces_constant.cu:288-369).  The algorithms here are this project's own:
// clusters are folded eagerly (no separate pending 2x2 per paired qubit), identity tests are EXACT
// (the reference's 1e-3 tolerance reorders gates), and level 3 groups clusters into
// cache-blocked passes by a greedy scan over the dependency order.
//
// Four files implement it, by concern (scheduler_impl.h holds the few helpers they share; libqsim.so exports none of them):
//   fusion.cpp        FusedOp predicates, the fusion algebra, the cluster state machine (add_1q / add_cx / add_2q / fold_2q /
//                     close / finish), the QSIM_SCHED_* knob table and engine_sched_config
//   tile_block.cpp    TileBlock methods, the row-class components, to_block, merge_blocks
//   pass_builder.cpp  single_op_pass, tile_pass, and the level-3 pass construction: PendingWalk (the ONE walk over the pending
//                     clusters) and PassBuilder, whose named steps build_passes calls in a loop
//   support_tracker.cpp  SupportTracker: the state's support as an affine subspace (affine.h), carried through the passes as they
//                     are handed out; what a tile pass over a partial support has to visit and may believe of its input (PassRegion)
#ifndef QSIM_SCHEDULER_H
#define QSIM_SCHEDULER_H

#include <algorithm>
#include <complex>
#include <cstdint>
#include <functional>
#include <vector>

#include "affine.h"
#include "qsim_internal.h"

namespace qsim {

using cd = std::complex<double>;

enum OpKind : int { OP_G1 = 1, OP_CX = 2, OP_G2 = 3 };

struct FusedOp {
    int kind = 0;
    int q_hi = -1;  // OP_G1: target; OP_CX: control; OP_G2: high qubit
    int q_lo = -1;  // OP_CX: target; OP_G2: low qubit
    cd m[16];       // row-major 2x2 / 4x4; index bits = (q_hi[, q_lo]), most significant first
    uint32_t gates = 0;

    int nq() const { return kind == OP_G1 ? 1 : 2; }
    int dim() const { return 1 << nq(); }
    uint64_t qmask() const {
        uint64_t m = 1ULL << q_hi;
        if (kind != OP_G1) m |= 1ULL << q_lo;
        return m;
    }
    bool is_diag() const;
    bool is_identity() const;
    uint64_t selector_mask() const; // qubits the matrix is block-diagonal in (exact zeros): it never mixes their 0 and 1 halves
};

// One block of a tile pass = one trip through LDS.  `q` are its qubits inside the tile; `s` are qubits OUTSIDE the tile
// that the block is block-diagonal in: constant over a tile, they only select which bank (sub-block on `q`) applies.
// nq == 0: a tile-uniform factor (entry (0,0) of each bank).  Stored by rows, at most kMaxRowNnz entries each: that is
// what one LDS trip of k_tile can evaluate (a dense 4x4 on two qubits is the fullest case), and it keeps the products
// of merge_blocks cheap on up to kMaxBlockQ qubits.
constexpr int kMaxBlockQ = 6, kMaxRowNnz = 4;
struct TileBlock {
    int nq = 0;
    int q[kMaxBlockQ] = {-1, -1, -1, -1, -1, -1}; // descending: q[0] is the most significant bit of the row/column index
    int ns = 0;
    int s[2] = {-1, -1};                      // descending: s[0] is the most significant bit of the bank index
    struct Row {
        int n = 0;
        uint8_t col[kMaxRowNnz];
        cd val[kMaxRowNnz];
        bool is_identity_row(int r) const { return n == 1 && col[0] == r && val[0] == cd(1.0, 0.0); } // row r of the identity, exactly
    };
    std::vector<Row> store; // banks() x dim() rows, bank-major; sized by shape()
    uint32_t gates = 0;

    void shape(int nq_, int ns_) { nq = nq_; ns = ns_; store.assign((size_t)1 << (nq_ + ns_), Row()); }
    Row &row(int v, int r) { return store[((size_t)v << nq) + r]; }
    const Row &row(int v, int r) const { return store[((size_t)v << nq) + r]; }

    int dim() const { return 1 << nq; }
    int banks() const { return 1 << ns; }
    uint64_t in_mask() const { uint64_t m = 0; for (int a = 0; a < nq; a++) m |= 1ULL << q[a]; return m; }
    uint64_t sel_mask() const { uint64_t m = 0; for (int a = 0; a < ns; a++) m |= 1ULL << s[a]; return m; }
    cd at(int v, int r, int c) const {
        const Row &rw = row(v, r);
        for (int j = 0; j < rw.n; j++)
            if (rw.col[j] == c) return rw.val[j];
        return cd(0, 0);
    }
    int max_row_nnz() const;    // over all banks
    bool bank_is_identity(int v) const;
    bool is_identity() const;   // every bank
    // the block as ONE matrix on the qubits (s..., q...), most significant first: block-diagonal in the bank index.
    // `out` holds (1 << (ns + nq))^2 entries.
    void full_matrix(cd *out) const;
    // Row classes (what one LDS trip of k_tile evaluates with ONE read per amplitude).  Per bank the nonzero pattern of a
    // block splits into connected components of rows and columns; in every block built from 1- and 2-qubit gates under
    // the kMaxRowNnz limit a component has as many columns as rows, at most kMaxRowNnz of each — the block is a direct
    // sum of small dense matrices in a permuted basis.  classes() packs the components of each bank into classes of
    // exactly T rows sharing exactly T columns (T = 1, 2 or 4, the same for all banks): rows[v] lists the rows class by
    // class, cols[v] the columns of class c at [c*T, (c+1)*T).  Identity rows are packed together so that whole classes
    // can be skipped.  false: some component is larger than kMaxRowNnz or the packing leaves a gap (such a block is
    // never built: merge_blocks asks first).
    bool classes(int &T, std::vector<std::vector<int>> &rows, std::vector<std::vector<int>> &cols) const;
    bool classes_feasible() const; // the answer of classes() without the layout, from the same components (no heap: merge_blocks asks often)
};

// tile_op.cpp: the block as the TileOp k_tile reads under geometry g.  false when a qubit is on the wrong side of the tile or the
// block cannot be expressed (Scheduler::merge_blocks never produces such a block).  f32: the state holds fp32 amplitudes — 8-byte
// LDS slots, coefficients rounded once, here, and stored as the float pairs the fp32 kernels consume (tile_kernel.inc coef_t).
bool to_tile_op(const TileGeom &g, const TileBlock &blk, TileOp &t, bool f32 = false);

// What SchedConfig::affine_support adds to a tile pass: where the pass has to go and what it may believe of its input, both
// from the affine subspace V of GF(2)^n that the state's support lies in when the pass starts (SupportTracker).
//   tiles    origin ^ span(gen): V projected onto the index bits outside the tile.  `refined`: that is fewer tiles than the
//            coordinate cube over (support | tile) which the pass visits otherwise; when it is not, gen are that cube's unit vectors.
//   checks   the region the PREVIOUS tile pass of the flush wrote when it was refined: an index outside it holds stale memory and
//            is staged in as zero.  Checks that the coordinate zero_mask of this pass implies are left out.
// visited / read_share are the shares of the register the pass then writes and reads; Pass::visited and Pass::read_share keep
// the coordinate count, which the plan probes and the pass-time model were fitted and pinned on.
constexpr int kMaxRegionGens = kAffineMaxGens, kMaxRegionChecks = kAffineMaxChecks; // what the kernel's record holds (qsim_internal.h TileAffine)
struct PassRegion {
    bool on = false;
    bool refined = false;
    uint64_t support_before = 0; // the coordinate support the engine must find when the pass starts: what all of this assumes
    uint64_t origin = 0;
    std::vector<uint64_t> gen;
    std::vector<ParityCheck> checks;
    double visited = 1.0, read_share = 1.0;
};

struct Pass {
    int kclass = 0;           // QSIM_K_*
    std::vector<FusedOp> ops;      // the one op of a single-op pass; empty for QSIM_K_TILE
    std::vector<TileBlock> blocks; // QSIM_K_TILE: geom.n_scale tile-uniform factors first, then the blocks in order
    TileGeom geom{};               // QSIM_K_TILE only
    uint32_t gates() const {
        uint32_t g = 0;
        for (const FusedOp &op : ops) g += op.gates;
        for (const TileBlock &b : blocks) g += b.gates;
        return g;
    }
    std::vector<uint32_t> src; // SchedConfig::track: the gates folded into this pass, by their order of arrival at the scheduler (0, 1, ...)
    double bytes = 0;         // algorithmic bytes this pass must move when it sweeps the whole register
    double visited = 1.0;     // ... times this: the fraction of the register inside the state's support after the pass (tile passes of a run that starts from a reset, SchedConfig::initial_support)
    double read_share = 1.0;  // tile passes of such a run: the fraction of the register the pass READS — of a visited tile only the slots inside the
                              // support before the pass are loaded (visited / 2^(tile qubits new to the support); 0 for the pass that generates the basis state)
    double moved() const { return bytes / 2 * (visited + read_share); } // algorithmic bytes of the pass as it runs: half of `bytes` are reads, half writes
    bool diag_full = false;   // QSIM_K_PHASE executed over every amplitude (d0 != 1 or q < 2)
    PassRegion region;        // SchedConfig::affine_support
};

// What a pass costs, in bytes moved at the rate of a pass that is bound by its memory traffic.  A tile pass is: up to four
// merged blocks hide behind the HBM time of the sweep, every further one adds 6.0 % of it (fp64; fp32 moves half the bytes per
// amplitude under the same blocks: 8.9 % from the fourth on).  Fitted on the tile passes of seven circuits under twelve scheduler
// settings at n = 30 with the kernel of the end of round 4 (tools/pass_model_data.py; profiles/r04/pass_model_n30_last_tree.csv, 1347 passes):
// ms = visited x (7.16 + 0.43 x max(0, blocks - 4)), rms error 0.43 ms (before the lanes walked conflict-free bits: 0.49 per block on the
// same settings; round 4's first fit 0.58, round 3's kernel 0.77); fp32 states (pass_model_n30_f32_last_tree.csv): 3.67 + 0.33 x
// max(0, blocks - 3), rms 0.24 ms (0.57 per block before the fp32 swizzle).  The planning steps (engine: which schedule; shard planner:
// which segmentation) rank by the sum of this — fewer sweeps are worth more than leaner ones, but not at any number of blocks.
// The byte term is the fitted one (bytes x visited), not Pass::moved(): a partial pass reads less than it writes since the
// kernel stopped loading slots outside the support, but the model was fitted on passes that loaded them, and which schedule a
// circuit gets hangs on it: it changes only together with a new fit.
inline double pass_time_cost(const Pass &p, bool f32) {
    if (p.kclass != QSIM_K_TILE) return p.bytes;
    const int nb = (int)p.blocks.size() - p.geom.n_scale;
    const int over = f32 ? (nb > 3 ? nb - 3 : 0) : (nb > 4 ? nb - 4 : 0);
    return p.bytes * p.visited * (1.0 + (f32 ? 0.089 : 0.060) * over);
}

struct SchedConfig {
    int n = 0;
    int fuse = 3;
    int tile_bits = 12;
    int tile_low_bits = 3;
    int tile_max_ops = 32;
    int tail_max_ops = 0;  // > tile_max_ops: the cap of a pass that can take ALL remaining clusters (no straggler pass for a handful of gates)
    int window = 512;  // clusters scanned ahead when grouping a pass
    int merge = 1;     // level 3: merge neighbouring blocks of a pass into sparse blocks of up to merge_qubits tile qubits
    int merge_qubits = 6; // round 4: 6 (64 rows = 8 parts of 8, one wave each in a 2^12 tile): 9 % fewer LDS trips than 5 at the same multiply-adds
    int rollout = 8;   // level 3: candidates tried (each by greedily finishing the pass) when a new qubit must be admitted; 0 = off
    int pad_from = 10; // first bit tried when unused tile slots are filled (below tile_low_bits: tile_low_bits)
    int lookahead = 0; // level 3: further passes (built greedily) whose reach is added to a candidate's score
    int local_iters = 0; // level 3: rounds of swap-one-qubit local search on each pass's qubit set
    int objective = 0; // what a pass maximises: 0 blocks, 1 source gates
    int selectors = 1; // level 3: a block may run in a pass whose tile lacks qubits it is block-diagonal in
    // Qubits that may already be 1 somewhere in the state when the first pass runs (all ones: unknown / dense).  After a
    // reset it is 0: a tile pass then only visits 2^(|support after it| - n) of the register (engine: qsim_state::support),
    // so while the support is small the scheduler (a) never takes a qubit outside it into a tile without need and (b)
    // first tries a pass that stays inside it altogether, keeping it when it absorbs more clusters than its share of a
    // full sweep is worth (cheap_margin x tile_max_ops x that share).
    uint64_t initial_support = ~0ULL;
    double cheap_margin = 1.0;
    // 1: a cluster may overtake an earlier pending one when both are block-diagonal in every qubit they share (they commute:
    // controls of CXs, diagonal gates); 0: any shared qubit orders them (round 1).  More freedom is better on average (ten
    // seeded 1000-gate circuits at n = 30: 892 -> 835 ms in total) but the greedy packing does not use it well on every
    // circuit, so the planning step (qsim_tune_circuit) schedules both ways and keeps the cheaper one for that circuit.
    int commute = 1;
    uint64_t seed = 0; // != 0: ties between equally good candidates (which cluster to admit next, which qubit to swap) are broken pseudo-randomly
                       // instead of in index order — another valid schedule of the same circuit per seed, for the planning step to choose among
    // > 0: while the support is partial (neither empty nor complete) the packer weighs its growth.  Every index bit a pass adds to the
    // support doubles the share of the register that pass and every later one visits, so a cluster that needs tile slots outside the
    // support ranks as if it needed support_weight more slots per such qubit (scan, the rollout candidates of grow_greedy), and the
    // local search scores a qubit set less support_weight per qubit outside it.  What fits a tile is still decided by the true slot
    // count.  0: the term is not evaluated at all — the schedule is what it was before the field existed.  Nothing changes on a dense
    // start or once the support is complete.  The planning step tries 5 and 10 beside 0 (choose_schedule).
    int support_weight = 0;
    // Level 3: 1 = X gates are not scheduled at all.  X only relabels the index, and it moves past any later gate exactly
    // (U X_q = X_q (X_q U X_q), the conjugate being U with rows and columns permuted), so the feed keeps a flip bit per qubit:
    // an exact X toggles it, an anti-diagonal 2x2 A is fed as the diagonal X A and toggles it, every other gate is fed conjugated
    // by the flips on its qubits.  What is left at the end is one mask m (Scheduler::residual_flips): the state is
    // psi[i] = psi'[i ^ m], which the caller owes — the engine has the stores of the last tile pass do it (k_tile PACK).  The X
    // gates then force no qubit into any tile.  Off by default: the constraints only ever shrink, but the greedy packing does
    // not turn that into fewer sweeps on every circuit, so it is one more variant for the planning step to price.
    int defer_flips = 0;
    // 1: every tile pass of a run that starts on a partial support carries its PassRegion.  The schedule itself is the same either
    // way: the packer keeps to the coordinate support.
    int affine_support = 0;
    int track = 0; // 1: every pass lists the gates it absorbed (Pass::src) — the shard planner asks which gates a segment's last pass holds
};

// The tile as the scheduler's steps see it, derived from the configuration in this one place.
struct TileShape {
    int B, L;          // index bits of a tile; the lowest L of them are always bits 0 .. L-1
    int kmax;          // free slots for high qubits
    uint64_t lowmask;  // bits 0 .. L-1
    // merge_blocks: tiles of fewer than 2^11 amplitudes keep to 3 qubits: a block on k > 3 qubits deals the 2^(k-3) parts of a group to
    // different waves, so a part must be at least one wave: 2^(B-k) >= 64 groups (k_tile's tile_op_part).  2^11 tiles take
    // 5 qubits, 2^12 and larger 6.
    int merge_max_q;
    explicit TileShape(const SchedConfig &c)
        : B(std::min(c.tile_bits, c.n)), L(std::min(c.tile_low_bits, B)), kmax(std::min(B - L, (int)kMaxTileHigh)), lowmask((1ULL << L) - 1ULL),
          merge_max_q(B >= 11 ? std::max(3, std::min(std::min(c.merge_qubits, kMaxBlockQ), B - 6)) : 3) {}
};

// The configuration qsim_flush schedules with for a state of n qubits (options as given by the caller; the search settings
// follow the size of the state, see the comment in fusion.cpp).
SchedConfig engine_sched_config(int n, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops, int pad_from = 10, bool f32 = false,
                                uint64_t initial_support = 0);

// The QSIM_SCHED_* environment variables override the search parameters for experiments (tools/).
// They are not part of the API and change the pass count, never the result — but they DO shape the schedule, so the
// engine folds this record into the identity of a cached plan (a plan built under one setting is never replayed under
// another).  `set` has one bit per variable that is present.  fusion.cpp's knob table is the ONE list of the variables: reading,
// applying and comparing all go over it.
struct SchedEnv {
    uint32_t set = 0;
    int lookahead = 0, rollout = 0, window = 0, local_iters = 0, objective = 0, merge = 0, merge_qubits = 0, cap = 0, seed = 0, support_weight = 0;
    double cheap_margin = 0;
    __attribute__((visibility("hidden"))) bool operator==(const SchedEnv &o) const;
};
SchedEnv read_sched_env();                      // the environment as it is now
void apply_sched_env(const SchedEnv &e, SchedConfig &cfg);

// The state's support as an affine subspace, carried through the passes of a schedule in the order they will run.  X translates
// it, CX maps it linearly, diagonal gates leave it alone; only a gate that mixes a qubit adds a direction, so its dimension grows
// by at most one per h / sx and not by one per qubit a tile touches.  Each merged block is applied by its exact non-zero pattern
// (the entries TileBlock keeps): the new V is the affine hull of every index some non-zero entry can carry an amplitude of V to.
// A hull may be larger than the true support (sound); it is never smaller.
class SupportTracker {
  public:
    void start(int n, uint64_t initial_support);
    void visit(Pass &p); // fills p.region (tile passes while the support is partial), then moves V through the pass
  private:
    void apply(const TileBlock &b);
    int n_ = 0;
    bool live_ = false;
    AffineSpace V_;
    uint64_t sup_ = 0;                // the coordinate support as the engine tracks it (qsim_state::support)
    std::vector<ParityCheck> wrote_;  // the region the last tile pass wrote, if it was refined
};

class Scheduler {
  public:
    explicit Scheduler(const SchedConfig &cfg);
    void add_1q(const cd U[4], int q);
    void add_cx(int control, int target);
    void add_2q(const cd U[16], int q_hi, int q_lo);
    // Closes every open cluster and produces the passes for everything added so far, in launch order.  The sink
    // form hands each pass over as soon as it is complete, so the caller can launch it while later passes are
    // still being scheduled.
    using PassSink = std::function<void(Pass &&)>;
    void finish(const PassSink &sink);
    void finish(std::vector<Pass> &out);
    uint64_t gates_seen() const { return gates_; }
    // SchedConfig::defer_flips: the index bits still flipped after everything added so far — the caller applies i -> i ^ mask to the
    // state the passes leave (0 when the option is off).  The deferred statements count with the last pass finish() hands out.
    uint64_t residual_flips() const { return flips_; }

    // fusion algebra, exposed for tests
    static void mul2(const cd a[4], const cd b[4], cd out[4]);     // out = a*b
    static void mul4(const cd a[16], const cd b[16], cd out[16]);  // out = a*b
    static void kron(const cd hi[4], const cd lo[4], cd out[16]);  // out = hi (x) lo
    static void cx4(bool control_is_hi, cd out[16]);

  private:
    SchedConfig cfg_;
    TileShape tile_;
    uint64_t gates_ = 0;
    std::vector<FusedOp> pool_;   // open clusters
    std::vector<int> open_;       // per qubit: index into pool_, or -1
    std::vector<FusedOp> closed_; // fused ops in a valid execution order
    std::vector<std::vector<uint32_t>> pool_src_, closed_src_; // SchedConfig::track: the gates behind pool_[i] / closed_[i]
    mutable std::vector<uint32_t> cur_src_;                     // ... and behind the pass being emitted
    SupportTracker tracker_;         // SchedConfig::affine_support
    uint64_t flips_ = 0;             // SchedConfig::defer_flips: qubits whose X is still owed
    std::vector<uint32_t> deferred_; // ... and the X statements that produced no cluster, by their order of arrival
    bool deferring() const { return cfg_.defer_flips != 0 && cfg_.fuse >= 3; }
    int flips_on(int q_hi, int q_lo) const { return (int)((flips_ >> q_hi & 1ULL) << 1 | (flips_ >> q_lo & 1ULL)); } // as a mask of a 4x4's row index

    class PassBuilder; // pass_builder.cpp: the state and the steps of build_passes
    void close(int idx);
    // the ONE way a cluster comes to be: opened on its qubits, or appended closed; `src`: the gates behind it (kept under SchedConfig::track)
    __attribute__((visibility("hidden"))) void open_cluster(const FusedOp &op, std::vector<uint32_t> src);
    __attribute__((visibility("hidden"))) void append_closed(const FusedOp &op, uint32_t gate_index);
    void fold_2q(const cd U[16], int q_hi, int q_lo, uint32_t gates, uint32_t gate_index);
    void build_passes(const PassSink &sink);
    void single_op_pass(const FusedOp &op, const PassSink &sink) const;
    // prefer: index bits free tile slots are filled from first (the state's support while it is partial); returns the tile's qubit mask
    uint64_t tile_pass(const std::vector<FusedOp> &ops, uint64_t hset, const PassSink &sink, uint64_t prefer = ~0ULL) const;
    void merge_blocks(std::vector<TileBlock> &blocks) const;
};

} // namespace qsim
#endif
