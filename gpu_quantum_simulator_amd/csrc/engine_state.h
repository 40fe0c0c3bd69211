// engine_state.h — what the host files of the engine share: the state behind the C ABI's qsim_state, the gate queue's record,
// the error channel, and the few internal functions that cross a file boundary.  Host only: the kernels include
// qsim_internal.h, never this.  Who defines what:
//   engine.cpp    errors, create / destroy, options, reset / support, the gate queue, launch_pass, the plan cache, the flush and
//                 the rule by which a flush schedules (flush_rule)
//   wisdom.cpp    the measured tile-bit orders and schedule choices (process-wide tables, private to it) and their file format
//   planning.cpp  the schedule choice per circuit and the timed planning (qsim_choose_schedule*, qsim_support_after, qsim_tune_circuit*)
//   plan_probe.cpp  the device-free probes of a circuit's schedule (qsim_plan_*, qsim_schedule_circuit*, qsim_tile_records);
//                 planning.h is what these three share
//   readout.cpp   reads, writes, norms, sampling                             pack.cpp  re-layouts and buffer hand-overs
//   profile.cpp   profiling events, statistics, the launch log              pauli.cpp  Pauli strings: expectation values, rotations
//                                                                           (controlled ones too) and adjoint gradients (the host
//                                                                           side of expect.hip, evolve.hip, crot.hip and
//                                                                           adjoint.hip; pauli_sweep.h), and the one owner of the
//                                                                           state's sweep scratch
//   state_algebra.cpp  calls on several states: copy, inner product, linear combination (the host side of combine.hip)
//   lanczos.cpp        the Lanczos ground-state solver on top of pauli.cpp's H application and the two above
//   density.cpp        reduced density matrices of qubit subsets: the plan, the call, from tiles to rho (the host side of density.hip; density.h)
//   subsystem.cpp      reduced density matrices of 6 to 10 qubits: the plan, the call, from blocks to rho (the host side of subsystem.hip; subsystem.h)
//   matrix.cpp         dense matrices on up to five targets under controls: the plan, the operand, the call (the host side of matrix.hip; matrix.h)
//   diagonal.cpp       whole-register diagonal operators from a table: the qsim_diagonal object, the plan, the set-up calls and the two sweeps (the host side of diagonal.hip; diagonal.h)
//   sample.cpp         shots drawn on the device: the pyramid's geometry and the call (the host side of sample.hip; sample.h)
//   qft.cpp            the quantum Fourier transform on any qubits: the plan, the per-pass record, the call (the host side of qft.hip; qft.h)
//   measure.cpp        projective measurement: post-selection, measurement by one draw of sample.cpp's sampler, the plan (the host side of measure.hip; measure.h)
#ifndef QSIM_ENGINE_STATE_H
#define QSIM_ENGINE_STATE_H

#include <atomic>
#include <thread>
#include <vector>

#include "circuit.h"
#include "qsim_internal.h"
#include "scheduler.h"

struct QueuedGate {
    int kind = 0, q0 = -1, q1 = -1;
    qsim::cd m[16];
    QueuedGate() = default;
    // U: the matrix as the C ABI passes it, row-major (re, im) pairs; not looked at for a CX
    QueuedGate(int kind_, int q0_, int q1_, const double *U) : kind(kind_), q0(q0_), q1(q1_) {
        for (int k = 0; U && k < mat_len(); k++) m[k] = qsim::cd(U[2 * k], U[2 * k + 1]);
    }
    // gate g of circuit c, as qsim_run_circuit queues it
    QueuedGate(const qsim_circuit &c, const qsim_gate_rec &g)
        : QueuedGate(g.kind, g.q0, g.kind == QSIM_GATE_U1 ? -1 : g.q1,
                     g.kind == QSIM_GATE_U1 ? c.mats2 + 8 * (long)g.mat : g.kind == QSIM_GATE_CX ? nullptr : c.mats4 + 32 * (long)g.mat) {}
    int mat_len() const { return kind == QSIM_GATE_U1 ? 4 : kind == QSIM_GATE_CX ? 0 : 16; } // entries of m that count
};

struct ProfEvent {
    hipEvent_t start, stop;
    int kclass;
    int n_ops;
    uint64_t high_mask;
    uint64_t order_code; // tile passes: the high tile bits in tile-local order, 5 bits each, lowest first
    double visited;      // tile passes: fraction of the register's tiles the pass works on (the state's support)
    double read_share;   // tile passes: fraction of the register the pass reads (the slots of those tiles inside the support before it)
    std::vector<uint8_t> forms; // tile passes: one byte per block (qsim_launch_log_blocks)
    std::vector<uint8_t> heads; // ... and five bytes per block out of the header of its encoded TileOp (qsim_launch_log_block_flags)
};
constexpr size_t kHeadBytes = 5;
struct LaunchRec { int kclass, n_ops; uint64_t high_mask; double ms; uint64_t order_code; double visited, read_share; std::vector<uint8_t> forms, heads; };

// Everything a schedule depends on: the options that shape it, the state's support, the QSIM_SCHED_* overrides and the
// gates themselves.  A cached plan is only replayed for a queue whose identity EQUALS the one it was built from, field by
// field and gate by gate; the 64-bit key merely finds the candidates (FNV-1a is not collision resistant, and "results
// identical to the reference" must not rest on a hash).
struct PlanIdentity {
    int opts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t support = 0;
    qsim::SchedEnv env;
    int defer = 0; // QSIM_OPT_DEFER_FLIPS as it applies to this flush (0: the flush may not defer X gates at all)
    int affine = 0; // QSIM_OPT_AFFINE_SUPPORT: the passes carry their PassRegion (compared, not hashed: the key names the same schedule either way)
    std::vector<QueuedGate> gates;
};

// How a flush schedules a queue of gates on a state that has a given support: the decisions flush_impl runs by, and what anything
// that predicts a flush (qsim_support_after for a cluster's exchanges, the key the planning step files a choice under) must go by.
struct FlushRule {
    bool cacheable = false; // the plan of this queue is kept and replayed (QSIM_OPT_PLAN_CACHE)
    bool hinted = false;    // a remembered schedule choice may apply to it
    int defer = 0;          // QSIM_OPT_DEFER_FLIPS as it applies to this flush (0: it may not defer X gates at all)
    uint64_t support = 0;   // where the state can be non-zero when the flush starts
    uint64_t key = 0;       // the queue's 64-bit name and the identity behind it (without the gates): only where cacheable or
    PlanIdentity id;        // hinted holds, or the caller asked for them
    // The scheduler's configuration: the hint applied, defer_flips settled.  Worked out on request — a replay schedules nothing.
    qsim::SchedConfig config(const qsim_state *s) const;
};

struct CachedPlan {
    uint64_t key = 0, wisdom_epoch = 0, last_use = 0;
    PlanIdentity id;
    std::vector<qsim::Pass> passes;
    std::vector<qsim::TileGeom> geoms;   // per pass; meaningful for tile passes: the geometry in the order it was launched with
    std::vector<size_t> op_first;  // per pass: index of its first TileOp in d_ops
    qsim::TileOp *d_ops = nullptr;
    uint64_t flip = 0;             // deferred X gates: the index flip the stores of the last tile pass apply (SchedConfig::defer_flips)
    std::vector<uint8_t> op_heads; // per TileOp of d_ops: kHeadBytes of its header (nq, terms, nsel, flags, b[7]), for the launch log
};

struct qsim_state {
    int n = 0, device = 0;
    hipStream_t stream = nullptr;
    void *amps = nullptr; // 2^n amplitudes: (re, im) pairs of double (16 B) or, with f32, of float (8 B)
    bool f32 = false;
    bool owns = false;
    // Second buffer of the same size for out-of-place tile passes (QSIM_OPT_PINGPONG; k_tile comment): a pass reads
    // `amps` and writes `spare`, then the two swap.  Within one qsim_flush an even number of passes run that way, so the
    // state is back in the buffer it started from when the flush returns (qsim_device_ptr stays what it was, an external
    // buffer holds the result).  Allocated on first use for states that own their buffer, or lent by the caller
    // (qsim_set_spare_buffer: a sharded run lends its exchange scratch, which is idle between exchanges).
    void *spare = nullptr;
    bool owns_spare = false, spare_failed = false;
    int pingpong = 1; // 0 never, 1 when the state is large enough to gain (kPingPongMinBytes), 2 whenever a second buffer can be had
    size_t amp_bytes() const { return f32 ? 8 : 16; }
    // options
    int fuse = 3, profile = 0, tile_bits = 12, tile_low_bits = 3, tile_max_ops = 32, grid_cap = 0, tile_threads = 0, tile_pad_from = 10, debug_tile_order = 0;
    uint64_t tile_passes = 0; // launched so far (seeds the probe permutations of QSIM_OPT_DEBUG_TILE_ORDER)
    long max_pending = 1L << 16;
    // queue
    std::vector<QueuedGate> queue;
    double zero_ket_amp = 1.0;     // amplitude at index 0 of the pending basis state (0: a shard that does not hold index 0)
    bool zero_ket_pending = false; // |0...0> requested but not written yet (folded into the first tile pass if possible)
    // After a reset the state is zero wherever an index bit outside `support` is set, and stays so until a pass mixes that
    // qubit in: the first tile pass writes ONE tile (every other tile is zero), the second 2^(tile qubits new to it)
    // tiles, and so on until the support is the whole register — typically the third pass of a random circuit.  While
    // `partial` is set, memory outside the support has never been written (it is zero by definition): tile passes visit
    // only tiles inside it and stage the rest of a tile in as zeros (launch_tile zero_mask); anything else that looks at
    // the buffer (other kernels, reads, exchanges) first gets the zeros written (materialize_zero_ket).
    bool partial = false;
    uint64_t support = 0; // qubits some tile pass has had inside its tile since the reset
    int sparse_start = 1; // QSIM_OPT_SPARSE_START
    // QSIM_OPT_AFFINE_SUPPORT: inside ONE flush the tile passes over a partial support go by the affine subspace the support lies in
    // (scheduler.h PassRegion): fewer tiles than the coordinate cube.  Between flushes the state is described by support / partial
    // alone: the last tile pass in front of anything that is not a tile pass of the same flush (a closing pass) writes the whole cube.
    int affine_support = 1;
    bool region_pending = false; // the last pass launched wrote only its region: the next launch must be a tile pass that tests it
    int defer_flips = 1;  // QSIM_OPT_DEFER_FLIPS
    uint64_t flips_applied = 0, flip_fallbacks = 0; // flushes whose last tile pass stored the state flipped; flushes that had to run the X gates as a pass of their own
    // op ring for tile passes
    qsim::TileOp *d_ops = nullptr, *h_ops = nullptr;
    size_t ops_cap = 0, ops_used = 0;
    double *d_expect = nullptr; // the sweep scratch: partial sums of a sweep, then the results of a batch of sweeps (alloc_sweep_scratch and the accessors below)
    void *d_adjoint = nullptr;  // qsim_pauli_gradient: lambda's 2^n amplitudes for a state without a spare buffer; allocated on first use, the state's own
    // stats
    qsim_stats stats{};
    std::vector<ProfEvent> events;      // recorded, not yet resolved
    std::vector<LaunchRec> launch_log;  // per-launch times since the last qsim_reset_stats (profile mode)
    std::vector<hipEvent_t> event_pool; // reusable
    // Plans of recently flushed gate queues (QSIM_OPT_PLAN_CACHE): the passes as scheduled, the tile passes' bit orders and
    // their TileOps resident on the device.  A queue that hashes to a cached plan is replayed launch by launch — no
    // scheduling, no block preparation, no H2D copy — which is what a loop that re-runs one circuit shape (a benchmark's
    // steps, a variational algorithm's iterations) pays for at n <= 26, where a pass is shorter than its planning.
    std::vector<struct CachedPlan> plans;
    uint64_t plan_clock = 0;
    int plan_cache = 1;
    int tune_schedules = 4; // qsim_tune_circuit: how many of the model's best schedules are run (QSIM_TUNE_SCHEDULES)
    long debug_plan_key = 0; // QSIM_OPT_DEBUG_PLAN_KEY: != 0 = every queue gets this key (forced collisions, for the tests of the identity check)
    uint64_t plan_hits = 0, plan_key_collisions = 0; // replays; key matches whose identity differed
    // qsim_create_async: the amplitude buffer is being allocated by this thread (hipMalloc of 16 GiB takes 0.04-0.25 s) while the
    // caller parses, sets options and chooses a schedule; whatever needs the buffer joins it first (await_buffer).
    std::thread alloc_thread;
    std::atomic<bool> alloc_done{true};
    hipError_t alloc_err = hipSuccess;
};

// The re-layout of an exchange done by the stores of the last tile pass in front of it (qsim_flush_pack; tile_kernel.inc k_tile PACK).
struct PackJob {
    qsim::PackMap map{};
    int bits[3] = {0, 0, 0};
    void *out = nullptr;    // where the caller wants the packed state (NULL: whichever of the state's two buffers it is not in)
    uint32_t skip = 0;      // blocks nobody will read (only the separate pack kernel leaves them out)
    uint64_t needed = ~0ULL; // source index bits that may be 1 where the receivers expect data
    void *packed_at = nullptr; // set when a tile pass did the re-layout: the buffer that now holds the packed state
};

namespace qsim {

// ---- engine.cpp ------------------------------------------------------------------------------------------------------------
// Sets the thread's message (qsim_last_error) and returns `code`: every host file of the engine reports through this one channel.
int fail(int code, const char *fmt, ...);
#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return qsim::fail(e_ == hipErrorOutOfMemory ? QSIM_ERR_ALLOC : QSIM_ERR_DEVICE, "%s failed: %s", #expr, \
                              hipGetErrorString(e_));                                                       \
    } while (0)
#define QSIM_TRY(expr) /* the same for a call that has reported its failure itself: returns its code */ \
    do {                                                                                                    \
        const int rc_ = (expr);                                                                             \
        if (rc_) return rc_;                                                                                \
    } while (0)
// What a kernel launcher returned, as the call's result: "<what> launch failed: <HIP's text>", out of memory as QSIM_ERR_ALLOC
int launched(const char *what, hipError_t e);
// The register a host-only plan probe is asked about: 0 to 40 qubits, precision_bits 64 or 32
int check_register_args(const char *who, int num_q, int precision_bits);
// QSIM_OK when both are there and the circuit has the state's number of qubits
int check_circuit(const qsim_state *s, const qsim_circuit *c);
// Joins the allocation of an asynchronously created state; QSIM_ERR_ALLOC ("Malloc error", quantum_simulator.c:170) if it failed.
int await_buffer(qsim_state *s);
// Writes the pending |0...0> with the init kernel (when the next operation cannot generate it itself), or the zeros of a
// state that has only been written inside its support so far.
int materialize_zero_ket(qsim_state *s);
// What every call that looks at the buffer opens with: the queued gates launched, then the zeros written (keep_partial: not those
// of a state that is written inside its support — the caller copes with it); settle() also makes the state's device current.
int written(qsim_state *s, bool keep_partial = false);
int settle(qsim_state *s, bool keep_partial = false);
// Qubits that may be 1 somewhere in the state when the next pass runs (SchedConfig::initial_support).
uint64_t current_support(const qsim_state *s);
// A caller's support as qsim_flush will key its plans with it: all ones for a dense state (or one that never starts sparse).
uint64_t plan_support(const qsim_state *s, uint64_t support);
// The scheduler configuration of the state's options, for a run that finds the state with this support (SchedConfig::initial_support).
SchedConfig state_sched_config(const qsim_state *s, uint64_t support);
void feed(Scheduler &sched, const std::vector<QueuedGate> &gates);
// The identity of a schedule without the gates, and its 64-bit name (the comment at their definitions).
PlanIdentity plan_identity(const qsim_state *s, size_t count, uint64_t support);
uint64_t gates_key(const qsim_state *s, const PlanIdentity &id, const QueuedGate *gates, size_t count);
// The second buffer for out-of-place tile passes, or NULL when the passes of this state run in place.
void *spare_buffer(qsim_state *s);
// Whether a plain flush of this state may leave its X gates to the stores of the last tile pass (QSIM_OPT_DEFER_FLIPS): level 3,
// fp64 in the tile shape that has the PACK variant, passes out of place between two buffers of the state's own.
bool may_defer_flips(qsim_state *s);
// Prepares the blocks of a tile pass for the given bit order in the pinned ring, uploads and launches them.
// affine / walk_gens: launch_tile's; a pass with a PassRegion always uploads its TileAffine record behind the blocks (a replay of
// the plan may need it where this launch does not).
int launch_tile_pass(qsim_state *s, const Pass &p, const TileGeom &geom, bool from_zero_ket, std::vector<TileOp> *capture = nullptr, bool oop = false,
                     uint64_t zero_mask = 0, PackJob *job = nullptr, uint64_t flip = 0, int affine = 0, int walk_gens = 0);
// qsim_flush; job != NULL: the last pass may write the state re-laid-out instead (PackJob, the comment at the definition).
int flush_impl(qsim_state *s, PackJob *job);
// How flush_impl will schedule these gates on a state with this support (for_pack: a flush with a PackJob).  want_key: key and
// identity are wanted whatever the flush would need them for.
FlushRule flush_rule(qsim_state *s, const std::vector<QueuedGate> &gates, uint64_t support, bool for_pack, bool want_key = false);
bool trace_pack(); // QSIM_TRACE_PACK is set: stderr says why a re-layout got a sweep of its own

// ---- wisdom.cpp (what the engine looks up; planning.h has what the planning step enters) ---------------------------------------
// Counts the tile pass and gives its high bits the measured order, if there is one (or the probe order of QSIM_OPT_DEBUG_TILE_ORDER).
// zero_mask: the index bits the state is zero in when the pass starts (0: a full or a generating pass) — the high bits among
// them end up topmost (place_new_bits), where the kernel drops their loads.
void order_tile_bits(qsim_state *s, TileGeom &g, uint64_t zero_mask = 0);
void place_new_bits(TileGeom &g, uint64_t zero_mask);
uint64_t wisdom_epoch(); // changes whenever a measured order or schedule choice does: cached plans carry the one they were built under
bool have_sched_hints();
void apply_sched_hint(uint64_t key, SchedConfig &cfg); // the schedule choice remembered under this key, if any

// ---- profile.cpp -----------------------------------------------------------------------------------------------------------
hipEvent_t take_event(qsim_state *s);

// ---- pauli.cpp: the state's sweep scratch, s->d_expect (pauli_sweep.h has its layout) -------------------------------------------
// Allocates it on first use, whoever calls first; qsim_destroy frees it.  The accessors want it allocated.
int alloc_sweep_scratch(qsim_state *s);
double *sweep_partials(qsim_state *s);      // kExpectPartialDoubles: what a reducing sweep takes as d_partial
double *sweep_result_row(qsim_state *s);    // the first of kResultRowBatch rows of kResultRowSlots sums: where a call of one sweep has it leave them
double *sweep_coef_staging(qsim_state *s);  // kMatrixCoefDoubles: the operand of qsim_apply_matrix (the definition says where it lies)
// matrix.cpp: `bytes` (at most kMatrixCoefDoubles doubles) through a pinned ring to sweep_coef_staging(s), ordered on the state's
// stream in front of the sweep that reads them; the operand of qsim_apply_matrix and of qsim_apply_permutation
int stage_sweep_operand(qsim_state *s, const void *data, size_t bytes);
// What qsim_destroy calls once it has waited for s->stream, before the stream goes.  The ring (matrix.cpp) and a table (diagonal.cpp)
// outlive a state and keep events last recorded on its stream; hipEventSynchronize looks at that stream, so an event must not be
// waited for after the stream died.  Everything on the stream has run by now: the slots are free and the reads are over.
void forget_staged_operands(const qsim_state *s);
void forget_diagonal_reads(const qsim_state *s);
// pauli.cpp: a second buffer of 2^n amplitudes for a call outside a flush (a gradient's lambda, a Fourier transform's moving passes):
// the idle spare buffer, else d_adjoint, allocated on first use.  QSIM_ERR_ALLOC when it cannot be had; nothing is touched then.
int second_buffer(qsim_state *s, void **out);
// out[0..count) = the first `count` sums of the first result row; waits for the state's stream
int fetch_sweep_results(qsim_state *s, int count, double *out);

// ---- sample.cpp ----------------------------------------------------------------------------------------------------------------
// qsim_sample_shots under the caller's name `who`: the same checks, the same pyramid, the same draws.  total (may be NULL): the sum
// the draws were scaled by, set whenever the pyramid was built.
int sample_outcomes(qsim_state *s, const char *who, const double *draws, long shots, const int *qubits, int num_qubits, uint64_t *out, double *total);

} // namespace qsim

struct LaunchScope { // records a start/stop pair around one launch when profiling is on
    qsim_state *s;
    ProfEvent pe{};
    bool on;
    LaunchScope(qsim_state *st, int kclass, int n_ops = 1, uint64_t high_mask = 0, uint64_t order_code = 0, double visited = 1.0, double read_share = 1.0) : s(st), on(st->profile != 0) {
        if (on) {
            pe.visited = visited;
            pe.read_share = read_share;
            pe.kclass = kclass;
            pe.n_ops = n_ops;
            pe.high_mask = high_mask;
            pe.order_code = order_code;
            pe.start = qsim::take_event(s);
            pe.stop = qsim::take_event(s);
            (void)hipEventRecord(pe.start, s->stream);
        }
    }
    ~LaunchScope() {
        if (on) {
            (void)hipEventRecord(pe.stop, s->stream);
            s->events.push_back(pe);
        }
    }
};

inline void account(qsim_state *s, int kclass, double bytes) {
    s->stats.launches++;
    s->stats.algorithmic_bytes += bytes;
    s->stats.k_launches[kclass]++;
    s->stats.k_bytes[kclass] += bytes;
}

#endif
