// engine.cpp — the core of the C ABI of include/qsim.h: errors, the device state and its options, the gate queue, the launch of
// a pass, the plan cache, the rule by which a flush schedules (flush_rule) and the flush that routes a queue's passes through the
// state's buffers.
// Host C++ compiled by hipcc for the HIP runtime API; every kernel lives in kernels.hip.  Owns qsim_state (engine_state.h) and
// the thread's error message; calls the scheduler, the launchers of qsim_internal.h and, in wisdom.cpp, the lookups of the
// measured tables (order_tile_bits, apply_sched_hint, have_sched_hints, wisdom_epoch).
//
// There is no CPU execution path in this file or anywhere in libqsim.so: if the HIP runtime reports no
// usable device, qsim_create() fails with QSIM_ERR_DEVICE.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "engine_state.h"

using namespace qsim;

// ---- errors --------------------------------------------------------------------------------------------
static thread_local std::string g_err; // the one definition: every file of the engine reports through fail()

int qsim::fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int qsim::launched(const char *what, hipError_t e) {
    if (e == hipSuccess) return QSIM_OK;
    return fail(e == hipErrorOutOfMemory ? QSIM_ERR_ALLOC : QSIM_ERR_DEVICE, "%s launch failed: %s", what, hipGetErrorString(e));
}

int qsim::check_register_args(const char *who, int num_q, int precision_bits) {
    if (num_q < 0 || num_q > 40) return fail(QSIM_ERR_ARG, "%s: a register of %d qubits", who, num_q);
    if (precision_bits != 64 && precision_bits != 32) return fail(QSIM_ERR_ARG, "%s: precision_bits is 64 or 32, not %d", who, precision_bits);
    return QSIM_OK;
}

extern "C" const char *qsim_last_error(void) { return g_err.c_str(); }

extern "C" int qsim_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// Makes `device` the thread's current one, or says why it cannot be.
static int use_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(QSIM_ERR_DEVICE, "no HIP device available (libqsim has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(QSIM_ERR_ARG, "device %d out of range (%d present)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    return QSIM_OK;
}

extern "C" int qsim_device_init(int device) {
    QSIM_TRY(use_device(device));
    HIP_TRY(hipFree(nullptr)); // forces context creation
    return QSIM_OK;
}

// ---- state ---------------------------------------------------------------------------------------------
int qsim::await_buffer(qsim_state *s) {
    if (s->alloc_thread.joinable()) s->alloc_thread.join();
    if (s->alloc_err != hipSuccess) {
        return fail(s->alloc_err == hipErrorOutOfMemory ? QSIM_ERR_ALLOC : QSIM_ERR_DEVICE, "Malloc error: %s (state needs %zu bytes)",
                    hipGetErrorString(s->alloc_err), s->amp_bytes() << s->n);
    }
    return QSIM_OK;
}

static constexpr size_t kOpsCap = 512;  // a pass holds <= tile_max_ops blocks; the ring wraps with a stream sync

static int make_state(qsim_state **out, int num_q, int device, void *ext, bool f32 = false, bool async = false) {
    if (!out) return fail(QSIM_ERR_ARG, "qsim_create: out is NULL");
    *out = nullptr;
    if (num_q < 0 || num_q > 40) return fail(QSIM_ERR_ARG, "qsim_create: %d qubits unsupported", num_q);
    QSIM_TRY(use_device(device));
    qsim_state *s = new qsim_state();
    s->n = num_q;
    s->device = device;
    s->f32 = f32;
    if (f32) { s->tile_bits = 13; s->tile_low_bits = 4; } // same 64 KiB of LDS per tile and the same 128-B runs as the fp64 default (64-B runs: 13 208 vs 14 130 gate-applies/s at n = 30)
    const size_t bytes = s->amp_bytes() << num_q;
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
        if (ext) s->amps = ext;
        else if (async) {
            s->owns = true;
            s->alloc_done.store(false);
            try {
                s->alloc_thread = std::thread([s, device, bytes]() {
                    hipError_t ae = hipSetDevice(device);
                    if (ae == hipSuccess) ae = hipMalloc(&s->amps, bytes);
                    if (ae != hipSuccess) { s->amps = nullptr; (void)hipGetLastError(); }
                    s->alloc_err = ae;
                    s->alloc_done.store(true);
                });
            } catch (...) { // no thread to be had: allocate here, like qsim_create
                s->alloc_done.store(true);
                e = hipMalloc(&s->amps, bytes);
                s->owns = (e == hipSuccess);
            }
        } else { e = hipMalloc(&s->amps, bytes); s->owns = (e == hipSuccess); }
    }
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_ops, kOpsCap * sizeof(TileOp));
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_ops, kOpsCap * sizeof(TileOp), hipHostMallocDefault);
    if (e != hipSuccess) {
        const int code = fail(e == hipErrorOutOfMemory ? QSIM_ERR_ALLOC : QSIM_ERR_DEVICE,
                              "Malloc error: %s (state needs %zu bytes)", hipGetErrorString(e), bytes);
        qsim_destroy(s);
        return code;
    }
    s->ops_cap = kOpsCap;
    *out = s;
    return qsim_reset(s);
}

extern "C" int qsim_create(qsim_state **out, int num_q, int device) { return make_state(out, num_q, device, nullptr); }
extern "C" int qsim_create_f32(qsim_state **out, int num_q, int device) { return make_state(out, num_q, device, nullptr, true); }
// The same with the amplitude buffer allocated on a helper thread: returns at once; gates may be queued, options set and a
// schedule chosen (qsim_choose_schedule_while_allocating) meanwhile, and the first call that needs the buffer waits for it.  An
// allocation failure surfaces there as QSIM_ERR_ALLOC.
extern "C" int qsim_create_async(qsim_state **out, int num_q, int device, int precision_bits) {
    if (precision_bits != 32 && precision_bits != 64) return fail(QSIM_ERR_ARG, "precision must be 32 or 64");
    return make_state(out, num_q, device, nullptr, precision_bits == 32, true);
}
extern "C" int qsim_precision_bits(const qsim_state *s) { return s ? (s->f32 ? 32 : 64) : -1; }
extern "C" int qsim_create_external(qsim_state **out, int num_q, int device, void *device_amps) {
    if (!device_amps) return fail(QSIM_ERR_ARG, "qsim_create_external: device_amps is NULL");
    return make_state(out, num_q, device, device_amps);
}

extern "C" void qsim_destroy(qsim_state *s) {
    if (!s) return;
    if (s->alloc_thread.joinable()) s->alloc_thread.join();
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    forget_staged_operands(s); // what outlives the state lets go of the events it recorded on this stream
    forget_diagonal_reads(s);
    for (auto &pe : s->events) { (void)hipEventDestroy(pe.start); (void)hipEventDestroy(pe.stop); }
    for (auto ev : s->event_pool) (void)hipEventDestroy(ev);
    for (CachedPlan &pl : s->plans)
        if (pl.d_ops) (void)hipFree(pl.d_ops);
    if (s->owns && s->amps) (void)hipFree(s->amps);
    if (s->owns_spare && s->spare) (void)hipFree(s->spare);
    if (s->d_ops) (void)hipFree(s->d_ops);
    if (s->h_ops) (void)hipHostFree(s->h_ops);
    if (s->d_expect) (void)hipFree(s->d_expect);
    if (s->d_adjoint) (void)hipFree(s->d_adjoint);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

extern "C" int qsim_num_qubits(const qsim_state *s) { return s ? s->n : -1; }
// The buffer as every queued gate left it: pending gates are launched and a lazily held |0...0> is written first (the
// work is ON the state's stream, not finished: order later accesses after qsim_stream() or call qsim_sync).
extern "C" void *qsim_device_ptr(qsim_state *s) {
    return s && written(s) == QSIM_OK ? s->amps : nullptr;
}
extern "C" void *qsim_stream(qsim_state *s) { return s ? (void *)s->stream : nullptr; }
// The buffer itself, nothing launched and nothing written first: for a caller that is about to overwrite (part of) it.
extern "C" void *qsim_state_buffer(qsim_state *s) { return s && await_buffer(s) == QSIM_OK ? s->amps : nullptr; }

extern "C" int qsim_set_option(qsim_state *s, int option, long value) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    if (!s->queue.empty()) {
        QSIM_TRY(qsim_flush(s)); // options apply to gates queued after the call
    }
    switch (option) {
    case QSIM_OPT_FUSE:
        if (value < 0 || value > 3) return fail(QSIM_ERR_ARG, "fuse level %ld not in 0..3", value);
        s->fuse = (int)value;
        break;
    case QSIM_OPT_PROFILE: s->profile = value < 0 ? 0 : value > 2 ? 2 : (int)value; break;
    case QSIM_OPT_TILE_BITS:
        if (value < 8 || value > 13) return fail(QSIM_ERR_ARG, "tile_bits %ld not in 8..13", value);
        s->tile_bits = (int)value;
        break;
    case QSIM_OPT_TILE_LOW_BITS:
        if (value < 2 || value > 6) return fail(QSIM_ERR_ARG, "tile_low_bits %ld not in 2..6", value);
        s->tile_low_bits = (int)value;
        break;
    case QSIM_OPT_MAX_PENDING:
        if (value < 1) return fail(QSIM_ERR_ARG, "max_pending must be positive");
        s->max_pending = value;
        break;
    case QSIM_OPT_TILE_MAX_OPS:
        if (value < 1 || value > (long)kOpsCap) return fail(QSIM_ERR_ARG, "tile_max_ops %ld not in 1..%zu", value, kOpsCap);
        s->tile_max_ops = (int)value;
        break;
    case QSIM_OPT_GRID_CAP:
        if (value < 0) return fail(QSIM_ERR_ARG, "grid_cap must be >= 0");
        s->grid_cap = (int)value;
        break;
    case QSIM_OPT_TILE_PAD_FROM:
        s->tile_pad_from = (int)value;
        break;
    case QSIM_OPT_DEBUG_TILE_ORDER:
        s->debug_tile_order = (int)value;
        break;
    case QSIM_OPT_PLAN_CACHE:
        s->plan_cache = value != 0;
        break;
    case QSIM_OPT_SPARSE_START:
        s->sparse_start = value != 0;
        break;
    case QSIM_OPT_AFFINE_SUPPORT:
        s->affine_support = value != 0;
        break;
    case QSIM_OPT_DEBUG_PLAN_KEY:
        s->debug_plan_key = value;
        break;
    case QSIM_OPT_DEFER_FLIPS:
        if (value < 0 || value > 2) return fail(QSIM_ERR_ARG, "defer_flips must be 0 (never), 1 (where the planned schedule says so) or 2 (wherever possible)");
        s->defer_flips = (int)value;
        break;
    case QSIM_OPT_PINGPONG:
        if (value < 0 || value > 2) return fail(QSIM_ERR_ARG, "pingpong must be 0 (never), 1 (auto) or 2 (always)");
        s->pingpong = (int)value;
        s->spare_failed = false;
        break;

    case QSIM_OPT_TILE_THREADS:
        if (value != 0 && value != 256 && value != 512 && value != 1024)
            return fail(QSIM_ERR_ARG, "tile_threads must be 0 (auto), 256, 512 or 1024");
        s->tile_threads = (int)value;
        break;
    default: return fail(QSIM_ERR_ARG, "unknown option %d", option);
    }
    return QSIM_OK;
}

extern "C" long qsim_get_option(const qsim_state *s, int option) {
    if (!s) return -1;
    switch (option) {
    case QSIM_OPT_FUSE: return s->fuse;
    case QSIM_OPT_PROFILE: return s->profile;
    case QSIM_OPT_TILE_BITS: return s->tile_bits;
    case QSIM_OPT_TILE_LOW_BITS: return s->tile_low_bits;
    case QSIM_OPT_MAX_PENDING: return s->max_pending;
    case QSIM_OPT_TILE_MAX_OPS: return s->tile_max_ops;
    case QSIM_OPT_GRID_CAP: return s->grid_cap;
    case QSIM_OPT_TILE_THREADS: return s->tile_threads;
    case QSIM_OPT_TILE_PAD_FROM: return s->tile_pad_from;
    case QSIM_OPT_DEBUG_TILE_ORDER: return s->debug_tile_order;
    case QSIM_OPT_PLAN_CACHE: return s->plan_cache;
    case QSIM_OPT_PINGPONG: return s->pingpong;
    case QSIM_OPT_SPARSE_START: return s->sparse_start;
    case QSIM_OPT_AFFINE_SUPPORT: return s->affine_support;
    case QSIM_OPT_DEBUG_PLAN_KEY: return s->debug_plan_key;
    case QSIM_OPT_DEFER_FLIPS: return s->defer_flips;
    default: return -1;
    }
}

int qsim::materialize_zero_ket(qsim_state *s) {
    QSIM_TRY(await_buffer(s));
    if (!s->zero_ket_pending && !s->partial) return QSIM_OK;
    if (s->region_pending) return fail(QSIM_ERR_ARG, "internal: the zeros of a state that was written inside an affine region only");
    HIP_TRY(hipSetDevice(s->device)); // a cluster drives several devices from one thread
    LaunchCfg cfg{s->stream, s->grid_cap};
    const double state_bytes = (double)s->amp_bytes() * (double)(1ULL << s->n);
    const bool whole = s->zero_ket_pending; // else only the part outside the support is written
    const uint64_t outside = index_mask(s->n) & ~s->support;
    s->zero_ket_pending = false;
    {
        LaunchScope scope(s, QSIM_K_INIT);
        HIP_TRY(whole ? launch_init(cfg, s->amps, s->f32, s->n, s->zero_ket_amp) : launch_zero_outside(cfg, s->amps, s->f32, s->n, outside));
    }
    account(s, QSIM_K_INIT, whole ? state_bytes : state_bytes * (1.0 - 1.0 / (double)(1ULL << __builtin_popcountll(outside))));
    s->partial = false;
    return QSIM_OK;
}

extern "C" int qsim_reset(qsim_state *s) { return qsim_reset_shard(s, 1); }

extern "C" int qsim_reset_shard(qsim_state *s, int holds_index0) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    HIP_TRY(hipSetDevice(s->device));
    s->queue.clear();
    s->zero_ket_amp = holds_index0 ? 1.0 : 0.0;
    // |0...0> is not written here: if the first pass after the reset is a tile pass it generates the state in LDS
    // (one write of the state instead of write + read + write); anything else materialises it first.
    s->zero_ket_pending = true;
    s->partial = false;
    s->support = 0;
    s->region_pending = false;
    return QSIM_OK;
}

// The caller filled the buffer itself (the receiving end of an exchange) and knows where the new contents can be non-zero:
// every amplitude whose index has a bit outside `support` is zero BY DEFINITION from now on (its memory need not have been
// written), exactly the situation after the first tile passes of a run (qsim_state::support).  Tile passes then visit only
// that part; anything else that looks at the buffer gets the zeros written first.
extern "C" int qsim_set_support(qsim_state *s, uint64_t support) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    QSIM_TRY(qsim_flush(s));
    const uint64_t nmask = index_mask(s->n);
    s->zero_ket_pending = false;
    s->support = support & nmask;
    s->partial = s->support != nmask;
    s->region_pending = false; // the caller describes the contents anew (a flush that failed behind a walking pass leaves it set)
    if (!s->sparse_start && s->partial) return materialize_zero_ket(s); // the option is off: keep the state dense
    return QSIM_OK;
}

// What the buffer holds right now, without touching it: *support = index bits that may be 1 in a written, possibly non-zero
// amplitude (all ones for a dense state); *kind = 0 written (inside the support), 1 a pending basis state amp0 * |0...0> that no
// kernel has written yet (amp0 = 0: the all-zero vector of a shard that holds nothing).  Queued gates are launched first.
extern "C" int qsim_get_support(qsim_state *s, uint64_t *support, int *kind, double *amp0) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    QSIM_TRY(qsim_flush(s));
    const uint64_t nmask = index_mask(s->n);
    if (support) *support = s->zero_ket_pending ? 0 : s->partial ? (s->support & nmask) : nmask;
    if (kind) *kind = s->zero_ket_pending ? 1 : 0;
    if (amp0) *amp0 = s->zero_ket_pending ? s->zero_ket_amp : 0.0;
    return QSIM_OK;
}

// 1 when the state is the all-zero vector of a shard that holds nothing (qsim_reset_shard(s, 0), nothing written since): gates
// queued on it change nothing, so the queue does not matter and nothing is flushed.
extern "C" int qsim_holds_nothing(const qsim_state *s) { return s && s->zero_ket_pending && s->zero_ket_amp == 0.0 ? 1 : 0; }

// ---- gate queue ----------------------------------------------------------------------------------------
// Checks the operands against the state (the matrix, if any, is in g already) and queues the gate.
static int enqueue(qsim_state *s, const QueuedGate &g) {
    const int n = s->n;
    if (g.kind == QSIM_GATE_U1) {
        if (g.q0 < 0 || g.q0 >= n) return fail(QSIM_ERR_ARG, "qubit %d out of range (n = %d)", g.q0, n);
    } else if (g.kind == QSIM_GATE_CX) {
        if (g.q0 < 0 || g.q0 >= n || g.q1 < 0 || g.q1 >= n) return fail(QSIM_ERR_ARG, "cx operands (%d, %d) out of range (n = %d)", g.q0, g.q1, n);
    } else if (g.q1 < 0 || g.q0 >= n || g.q1 >= g.q0) {
        return fail(QSIM_ERR_ARG, "2q operands need 0 <= q_lo < q_hi < n (got %d, %d, n = %d)", g.q0, g.q1, n);
    }
    s->queue.push_back(g);
    s->stats.gates++;
    if ((long)s->queue.size() >= s->max_pending) return qsim_flush(s);
    return QSIM_OK;
}

extern "C" int qsim_apply_1q(qsim_state *s, const double *U, int target) {
    if (!s || !U) return fail(QSIM_ERR_ARG, "NULL argument");
    return enqueue(s, QueuedGate(QSIM_GATE_U1, target, -1, U));
}

extern "C" int qsim_apply_cx(qsim_state *s, int control, int target) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    return enqueue(s, QueuedGate(QSIM_GATE_CX, control, target, nullptr));
}

extern "C" int qsim_apply_2q(qsim_state *s, const double *U, int q_hi, int q_lo) {
    if (!s || !U) return fail(QSIM_ERR_ARG, "NULL argument");
    return enqueue(s, QueuedGate(QSIM_GATE_U2, q_hi, q_lo, U));
}

extern "C" int qsim_scale(qsim_state *s, double re, double im) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    if (s->n < 1) return fail(QSIM_ERR_ARG, "scale needs at least one local qubit");
    const double U[8] = {re, im, 0, 0, 0, 0, re, im}; // diag(z, z) on local qubit 0: folds into the next fused block
    return qsim_apply_1q(s, U, 0);
}

int qsim::check_circuit(const qsim_state *s, const qsim_circuit *c) {
    if (!s || !c) return fail(QSIM_ERR_ARG, "NULL argument");
    if (c->num_q != s->n) return fail(QSIM_ERR_ARG, "circuit has %d qubits, state has %d", c->num_q, s->n);
    return QSIM_OK;
}

extern "C" int qsim_run_circuit(qsim_state *s, const qsim_circuit *c, long first, long count) {
    QSIM_TRY(check_circuit(s, c));
    if (first < 0 || first > c->count) return fail(QSIM_ERR_ARG, "first gate %ld outside the circuit", first);
    long end = count < 0 ? c->count : first + count;
    if (end > c->count) end = c->count;
    for (long i = first; i < end; i++) {
        QSIM_TRY(enqueue(s, QueuedGate(*c, c->gates[i])));
    }
    return QSIM_OK;
}

// ---- scheduling + launch -------------------------------------------------------------------------------
SchedConfig qsim::state_sched_config(const qsim_state *s, uint64_t support) {
    return engine_sched_config(s->n, s->fuse, s->tile_bits, s->tile_low_bits, s->tile_max_ops, s->tile_pad_from, s->f32, support);
}
uint64_t qsim::plan_support(const qsim_state *s, uint64_t support) {
    const uint64_t nmask = index_mask(s->n);
    return !s->sparse_start || (support & nmask) == nmask ? ~0ULL : support & nmask;
}

void qsim::feed(Scheduler &sched, const std::vector<QueuedGate> &gates) {
    for (const QueuedGate &g : gates) {
        if (g.kind == QSIM_GATE_U1) sched.add_1q(g.m, g.q0);
        else if (g.kind == QSIM_GATE_CX) sched.add_cx(g.q0, g.q1);
        else sched.add_2q(g.m, g.q0, g.q1);
    }
}

static inline void to_m2(const FusedOp &op, M2 &u) {
    for (int k = 0; k < 4; k++) { u.re[k] = op.m[k].real(); u.im[k] = op.m[k].imag(); }
}
static inline void to_m4(const FusedOp &op, M4 &u) {
    for (int k = 0; k < 16; k++) { u.re[k] = op.m[k].real(); u.im[k] = op.m[k].imag(); }
}

// The second buffer is worth its memory from this size on.
// measured (bench circuits, same box, alternating runs): n = 24 -12 %, n = 25..28 +-0.2 %, n = 29 +1.4 %, n = 30 +1.6 %, n = 31 +1.5 %
constexpr size_t kPingPongMinBytes = (size_t)8 << 30;
void *qsim::spare_buffer(qsim_state *s) {
    const size_t bytes = s->amp_bytes() << s->n;
    if (s->pingpong == 0 || (s->pingpong == 1 && bytes < kPingPongMinBytes)) return nullptr;
    if (s->spare) return s->spare;
    if (!s->owns || s->spare_failed) return nullptr; // an external buffer is only ever paired with a lent one
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + total_b / 16 ||
        hipMalloc(&s->spare, bytes) != hipSuccess) {
        (void)hipGetLastError();
        s->spare = nullptr;
        s->spare_failed = true; // not enough memory for two copies: stay in place, do not ask again
        return nullptr;
    }
    s->owns_spare = true;
    return s->spare;
}

// Launches a tile pass whose TileOps are already on the device (no statistics, no profiling events).  oop: write the
// state to the spare buffer and make that the state (the caller checked spare_buffer()).  job: the pass writes the state,
// re-laid-out, to job->out (or the buffer the state is not in) and records where.
// flip (with oop, without job): deferred X gates — the amplitude of index i is stored at i ^ flip of the spare buffer.
static int launch_tile_prepared(qsim_state *s, const TileGeom &geom, const TileOp *d, int need, bool from_zero_ket, bool oop = false, uint64_t zero_mask = 0,
                                PackJob *job = nullptr, uint64_t flip = 0, int affine = 0, int walk_gens = 0) {
    LaunchCfg cfg{s->stream, s->grid_cap};
    const int threads = s->tile_threads; // 0: default for the tile size
    if (job) {
        void *dst = job->out ? job->out : (s->spare && s->spare != s->amps ? s->spare : nullptr);
        if (!dst || dst == s->amps) return fail(QSIM_ERR_ARG, "internal: no buffer for the re-layout");
        const hipError_t e = launch_tile(cfg, s->amps, dst, s->f32, geom, d, need, threads, from_zero_ket, s->zero_ket_amp, zero_mask, &job->map, affine, walk_gens);
        if (e != hipSuccess) return fail(QSIM_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
        job->packed_at = dst;
        return QSIM_OK;
    }
    PackMap flips = identity_pack_map();
    flips.flip = flip;
    if (flip && (!oop || !s->spare || s->spare == s->amps)) return fail(QSIM_ERR_ARG, "internal: deferred flips need an out-of-place pass");
    const hipError_t e = launch_tile(cfg, s->amps, oop ? s->spare : s->amps, s->f32, geom, d, need, threads, from_zero_ket, s->zero_ket_amp, zero_mask, flip ? &flips : nullptr, affine, walk_gens);
    if (e != hipSuccess) return fail(QSIM_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
    if (oop) std::swap(s->amps, s->spare);
    return QSIM_OK;
}

// Prepares the blocks of a tile pass for the given bit order in the pinned ring, uploads and launches them; `capture`
// (optional) receives a copy of the prepared TileOps for the plan cache.
// The TileAffine record of a pass's region, in the place of a TileOp (zeroed beyond it).
static void encode_region(const PassRegion &r, TileOp &slot) {
    memset(&slot, 0, sizeof slot);
    TileAffine a{};
    a.origin = r.origin;
    a.n_gen = (uint32_t)std::min(r.gen.size(), (size_t)kAffineMaxGens);
    for (uint32_t j = 0; j < a.n_gen; j++) a.gen[j] = r.gen[j];
    a.n_chk = (uint32_t)std::min(r.checks.size(), (size_t)kAffineMaxChecks);
    for (uint32_t j = 0; j < a.n_chk; j++) { a.chk[j] = r.checks[j].mask; a.chk_par |= (uint32_t)(r.checks[j].parity & 1) << j; }
    memcpy(&slot, &a, sizeof a);
}
// TileOps a pass takes in the op buffer: its blocks, and behind them the record of its region
static size_t pass_op_slots(const Pass &p) { return p.blocks.size() + (p.region.on ? 1 : 0); }

int qsim::launch_tile_pass(qsim_state *s, const Pass &p, const TileGeom &geom, bool from_zero_ket, std::vector<TileOp> *capture, bool oop, uint64_t zero_mask,
                           PackJob *job, uint64_t flip, int affine, int walk_gens) {
    const size_t blocks = p.blocks.size(), need = pass_op_slots(p);
    if (need > s->ops_cap) return fail(QSIM_ERR_ARG, "tile pass with %zu ops exceeds the op buffer", need);
    if (s->ops_used + need > s->ops_cap) { // ring is full: wait until earlier passes have read their ops
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->ops_used = 0;
    }
    TileOp *h = s->h_ops + s->ops_used;
    for (size_t k = 0; k < blocks; k++)
        if (!to_tile_op(geom, p.blocks[k], h[k], s->f32)) return fail(QSIM_ERR_ARG, "internal: block does not fit its tile pass");
    if (need > blocks) encode_region(p.region, h[blocks]);
    if (capture) capture->insert(capture->end(), h, h + need);
    TileOp *d = s->d_ops + s->ops_used;
    HIP_TRY(hipMemcpyAsync(d, h, need * sizeof(TileOp), hipMemcpyHostToDevice, s->stream));
    s->ops_used += need;
    return launch_tile_prepared(s, geom, d, (int)blocks, from_zero_ket, oop, zero_mask, job, flip, affine, walk_gens);
}

// cached_geom / cached_ops: replay of a cached plan (the tile pass's order and device-resident TileOps);
// capture / geom_out: the first run of a plan records them.
// The five header bytes of an encoded block that say which form of the kernel it runs through (qsim_launch_log_block_flags).
static void push_head(std::vector<uint8_t> &out, const TileOp &t) {
    for (uint8_t byte : {t.nq, t.terms, t.nsel, t.flags, t.b[7]}) out.push_back(byte);
}

// cached_heads: those bytes of the cached records, kept on the host with the plan (kHeadBytes per op).
static int launch_pass(qsim_state *s, const Pass &p, const TileGeom *cached_geom = nullptr, const TileOp *cached_ops = nullptr,
                       std::vector<TileOp> *capture = nullptr, TileGeom *geom_out = nullptr, bool oop = false, PackJob *job = nullptr,
                       const uint8_t *cached_heads = nullptr, uint64_t flip = 0, bool closing = true) {
    const bool from_zero_ket = s->zero_ket_pending && p.kclass == QSIM_K_TILE;
    if (s->region_pending && p.kclass != QSIM_K_TILE) return fail(QSIM_ERR_ARG, "internal: a kernel other than a tile pass behind a pass that was not closing");
    if ((s->zero_ket_pending || s->partial) && p.kclass != QSIM_K_TILE) { // only tile passes work on a partially written state
        QSIM_TRY(materialize_zero_ket(s));
    }
    s->zero_ket_pending = false;
    LaunchCfg cfg{s->stream, s->grid_cap};
    const FusedOp &op = p.ops[0];
    hipError_t e = hipSuccess;
    double visited = 1.0;    // fraction of the tiles a tile pass works on = the share of the register it writes
    double read_share = 1.0; // the share of the register it reads
    switch (p.kclass) {
    case QSIM_K_GATE1:
    case QSIM_K_GATE1_LO: {
        M2 u;
        to_m2(op, u);
        LaunchScope scope(s, p.kclass);
        e = launch_gate1(cfg, s->amps, s->f32, s->n, op.q_hi, u);
        break;
    }
    case QSIM_K_PHASE: {
        LaunchScope scope(s, p.kclass);
        if (p.diag_full)
            e = launch_diag1_full(cfg, s->amps, s->f32, s->n, op.q_hi, op.m[0].real(), op.m[0].imag(), op.m[3].real(),
                                  op.m[3].imag());
        else
            e = launch_phase(cfg, s->amps, s->f32, s->n, op.q_hi, op.m[3].real(), op.m[3].imag());
        break;
    }
    case QSIM_K_CX: {
        LaunchScope scope(s, p.kclass);
        e = launch_cx(cfg, s->amps, s->f32, s->n, op.q_hi, op.q_lo);
        break;
    }
    case QSIM_K_GATE2: {
        M4 u;
        to_m4(op, u);
        LaunchScope scope(s, p.kclass);
        e = launch_gate2(cfg, s->amps, s->f32, s->n, op.q_hi, op.q_lo, u);
        break;
    }
    case QSIM_K_TILE: {
        TileGeom geom = cached_geom ? *cached_geom : p.geom;
        // the part of the register this pass has to visit (qsim_state::support)
        const uint64_t nmask = index_mask(s->n);
        const uint64_t tmask = tile_mask(geom);
        uint64_t zero_mask = 0;
        if (s->sparse_start && from_zero_ket) zero_mask = nmask;
        else if (s->partial) zero_mask = nmask & ~s->support;
        // (a cached plan was recorded on the same support: its order has the new bits where this one puts them)
        if (!cached_geom) order_tile_bits(s, geom, from_zero_ket ? 0 : zero_mask);
        if (geom_out) *geom_out = geom;
        uint64_t hm = 0, oc = 0;
        for (int j = 0; j < geom.n_high; j++) { hm |= 1ULL << geom.high[j]; oc |= (uint64_t)geom.high[j] << (5 * j); }
        visited = 1.0 / (double)(1ULL << __builtin_popcountll(zero_mask & ~tmask));
        // of a visited tile only the slots inside the support are read (k_tile SPARSE); a generating pass reads nothing
        read_share = from_zero_ket ? 0.0 : visited / (double)(1ULL << __builtin_popcountll(zero_mask & tmask));
        // QSIM_OPT_AFFINE_SUPPORT: the pass goes by its region where that says what this launch finds — a partially written state of
        // exactly the support the scheduler assumed.  It tests its input by the previous pass's region if that pass wrote nothing
        // else, and walks its own tiles unless it is closing (the next thing to run is no tile pass of this flush that tests them).
        const PassRegion &reg = p.region;
        const bool by_region = s->affine_support && reg.on && zero_mask != 0 && !from_zero_ket && (reg.support_before & nmask) == (s->support & nmask);
        if (s->region_pending && !(by_region && !reg.checks.empty()))
            return fail(QSIM_ERR_ARG, "internal: a tile pass without the checks of the region the pass before it wrote");
        int affine = 0, walk_gens = 0;
        if (by_region) {
            if (s->region_pending) affine |= kAffineChecks;
            if (!closing && reg.refined && reg.gen.size() <= (size_t)kAffineMaxGens) {
                affine |= kAffineWalk;
                walk_gens = (int)reg.gen.size();
                visited = reg.visited;
                read_share = reg.read_share;
            }
        }
        LaunchScope scope(s, p.kclass, (int)p.blocks.size(), hm, oc, visited, read_share);
        if (scope.on && s->profile >= 2) // what the blocks look like, for the pass-time model's data (tools/pass_model_data.py); host work per launch: only on request
            for (size_t k = (size_t)geom.n_scale; k < p.blocks.size(); k++) {
                const TileBlock &b = p.blocks[k];
                int T = 0;
                std::vector<std::vector<int>> rows, cols;
                if (!b.classes(T, rows, cols)) T = 4;
                int ident = 0; // rows that are identity in every bank
                for (int r = 0; r < b.dim(); r++) {
                    bool id = true;
                    for (int v = 0; v < b.banks() && id; v++) { const auto &rw = b.row(v, r); id = rw.n == 1 && rw.col[0] == r && rw.val[0] == cd(1, 0); }
                    ident += id;
                }
                scope.pe.forms.push_back((uint8_t)((T == 4 ? 2 : T == 2 ? 1 : 0) | (b.nq << 2) | (2 * ident >= b.dim() ? 32 : 0) | (b.ns << 6)));
            }
        const int rc = cached_ops ? launch_tile_prepared(s, geom, cached_ops, (int)p.blocks.size(), from_zero_ket, oop, zero_mask, job, flip, affine, walk_gens)
                                  : launch_tile_pass(s, p, geom, from_zero_ket, capture, oop, zero_mask, job, flip, affine, walk_gens);
        if (rc) return rc;
        s->region_pending = (affine & kAffineWalk) != 0;
        if (scope.on && s->profile >= 2) { // which kernel form each block ran through: out of the records the kernel was given
            const size_t need = p.blocks.size();
            const TileOp *h = s->h_ops + (s->ops_used - pass_op_slots(p)); // a fresh pass: launch_tile_pass has just encoded them there
            for (size_t k = (size_t)geom.n_scale; k < need; k++) {
                if (!cached_ops) push_head(scope.pe.heads, h[k]);
                else if (cached_heads) scope.pe.heads.insert(scope.pe.heads.end(), cached_heads + kHeadBytes * k, cached_heads + kHeadBytes * (k + 1));
            }
        }
        if (zero_mask) {
            s->support = (from_zero_ket ? 0 : s->support) | tmask;
            s->partial = (s->support & nmask) != nmask;
        }
        break;
    }
    default: return fail(QSIM_ERR_ARG, "internal: unknown kernel class %d", p.kclass);
    }
    if (e != hipSuccess) return fail(QSIM_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
    const double scale = s->f32 ? 0.5 : 1.0; // the scheduler prices passes for 16-byte amplitudes
    account(s, p.kclass, scale * p.bytes / 2 * (visited + read_share)); // half of a pass's bytes are reads, half writes
    return QSIM_OK;
}

uint64_t qsim::current_support(const qsim_state *s) {
    if (!s->sparse_start) return ~0ULL;
    if (s->zero_ket_pending) return 0;
    return s->partial ? s->support : ~0ULL;
}

// The identity of a schedule (PlanIdentity) without the gates, and its 64-bit name: FNV-1a over the options that shape a
// plan, the state's support, the QSIM_SCHED_* overrides and every gate.  The key only FINDS cached plans and scheduler
// hints; a plan is replayed only after plan_matches() has compared the identity itself.
PlanIdentity qsim::plan_identity(const qsim_state *s, size_t count, uint64_t support) {
    PlanIdentity id;
    const int opts[8] = {s->n, s->f32 ? 1 : 0, s->fuse, s->tile_bits, s->tile_low_bits, s->tile_max_ops, s->tile_pad_from, (int)count};
    memcpy(id.opts, opts, sizeof opts);
    id.support = support; // the schedule depends on where the state is known to be zero
    id.env = read_sched_env();
    return id;
}
uint64_t qsim::gates_key(const qsim_state *s, const PlanIdentity &id, const QueuedGate *gates, size_t count) {
    if (s->debug_plan_key) return (uint64_t)s->debug_plan_key;
    uint64_t h = 0xcbf29ce484222325ULL;
    auto mix = [&](const void *p, size_t n) {
        const unsigned char *b = (const unsigned char *)p;
        for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ULL; }
    };
    mix(id.opts, sizeof id.opts);
    mix(&id.support, sizeof id.support);
    const int env_i[9] = {(int)id.env.set, id.env.lookahead, id.env.rollout, id.env.window, id.env.local_iters, id.env.objective, id.env.merge, id.env.merge_qubits, id.env.cap};
    mix(env_i, sizeof env_i);
    mix(&id.env.cheap_margin, sizeof id.env.cheap_margin);
    for (size_t i = 0; i < count; i++) {
        const QueuedGate &g = gates[i];
        const int hd[3] = {g.kind, g.q0, g.q1};
        mix(hd, sizeof hd);
        mix(g.m, g.mat_len() * sizeof(cd));
    }
    return h;
}
static bool same_gates(const QueuedGate *a, const QueuedGate *b, size_t count) {
    for (size_t i = 0; i < count; i++) {
        if (a[i].kind != b[i].kind || a[i].q0 != b[i].q0 || a[i].q1 != b[i].q1) return false;
        if (memcmp(a[i].m, b[i].m, a[i].mat_len() * sizeof(cd)) != 0) return false;
    }
    return true;
}
static bool plan_matches(const PlanIdentity &have, const PlanIdentity &want, const QueuedGate *gates, size_t count) {
    return memcmp(have.opts, want.opts, sizeof have.opts) == 0 && have.support == want.support && have.env == want.env && have.defer == want.defer && have.affine == want.affine &&
           have.gates.size() == count && same_gates(have.gates.data(), gates, count);
}

bool qsim::trace_pack() {
    static const bool on = getenv("QSIM_TRACE_PACK") != nullptr;
    return on;
}

// A tile pass can take the re-layout on board when the kernel has that variant for its shape (fp64, 2^12-amplitude tiles, 512
// threads) and when what it writes covers what the receivers will look at: a pass over a partially written state only
// visits the tiles inside (support | its own tile bits), so source indices outside that never reach the output — fine as
// long as job->needed (where the receivers expect data) lies inside it; else the pack kernel does the job (it writes zeros).
// support_before: where the state can be non-zero when the pass starts (current_support() once every earlier pass has been launched).
static bool pass_can_pack(const qsim_state *s, const Pass *p, const TileGeom &geom, const PackJob *job, uint64_t support_before) {
    const bool trace = trace_pack();
    if (!p || p->kclass != QSIM_K_TILE || !launch_tile_can_pack(s->f32, geom, s->tile_threads)) {
        if (trace) fprintf(stderr, "qsim: re-layout not fused: last pass is %s\n", !p || p->kclass != QSIM_K_TILE ? "no tile pass" : "a tile pass without the packing variant");
        return false;
    }
    const uint64_t nmask = index_mask(s->n);
    const uint64_t after = tile_mask(geom) | support_before;
    if (trace && ((job->needed & nmask) & ~after) != 0)
        fprintf(stderr, "qsim: re-layout not fused: the pass writes support %llx, the receivers look at %llx\n", (unsigned long long)(after & nmask), (unsigned long long)(job->needed & nmask));
    return ((job->needed & nmask) & ~after) == 0;
}

// ---- plan cache ----------------------------------------------------------------------------------------
constexpr size_t kMaxPlans = 8, kMaxCachedOps = 4096;

// The cached plan of exactly this queue, built under the tables as they are now (epoch), or NULL.
static CachedPlan *find_plan(qsim_state *s, uint64_t key, uint64_t epoch, const PlanIdentity &ident) {
    for (CachedPlan &pl : s->plans) {
        if (pl.key != key || pl.wisdom_epoch != epoch) continue;
        if (!plan_matches(pl.id, ident, s->queue.data(), s->queue.size())) { s->plan_key_collisions++; continue; } // same name, other circuit
        s->plan_hits++;
        pl.last_use = ++s->plan_clock;
        return &pl;
    }
    return nullptr;
}

namespace {
// What the fresh path of a flush records for the plan cache while its passes are launched: the passes, the geometry each tile
// pass was launched with and its TileOps.
struct PlanRecorder {
    CachedPlan plan;
    std::vector<TileOp> host_ops;
    int launch(qsim_state *s, Pass &&p, bool oop, PackJob *job, uint64_t flip, bool closing);
};

// Keeps the recorded plan: its TileOps move to a device buffer of their own (one copy, ordered behind the launches).  A stale plan
// of the same queue (the geometry table changed) is replaced, else the least recently used one once kMaxPlans are held.
static int keep_plan(qsim_state *s, PlanRecorder &rec, uint64_t key, uint64_t epoch) {
    CachedPlan &fresh = rec.plan;
    if (rec.host_ops.size() > kMaxCachedOps) return QSIM_OK;
    if (!rec.host_ops.empty()) {
        if (hipMalloc((void **)&fresh.d_ops, rec.host_ops.size() * sizeof(TileOp)) != hipSuccess) { (void)hipGetLastError(); return QSIM_OK; }
        if (hipMemcpy(fresh.d_ops, rec.host_ops.data(), rec.host_ops.size() * sizeof(TileOp), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(fresh.d_ops);
            (void)hipGetLastError();
            return QSIM_OK;
        }
    }
    for (const TileOp &t : rec.host_ops) push_head(fresh.op_heads, t); // (the records themselves live on the device only)
    fresh.key = key;
    fresh.wisdom_epoch = epoch;
    fresh.last_use = ++s->plan_clock;
    size_t slot = s->plans.size();
    for (size_t i = 0; i < s->plans.size(); i++)
        if (s->plans[i].key == key && plan_matches(s->plans[i].id, fresh.id, fresh.id.gates.data(), fresh.id.gates.size())) slot = i;
    if (slot == s->plans.size() && s->plans.size() >= kMaxPlans) {
        slot = 0;
        for (size_t i = 1; i < s->plans.size(); i++)
            if (s->plans[i].last_use < s->plans[slot].last_use) slot = i;
    }
    if (slot < s->plans.size()) {
        if (s->plans[slot].d_ops) {
            HIP_TRY(hipStreamSynchronize(s->stream)); // a replay of the evicted plan may still be reading its ops
            (void)hipFree(s->plans[slot].d_ops);
        }
        s->plans[slot] = std::move(fresh);
    } else {
        s->plans.push_back(std::move(fresh));
    }
    return QSIM_OK;
}

int PlanRecorder::launch(qsim_state *s, Pass &&p, bool oop, PackJob *job, uint64_t flip, bool closing) {
    TileGeom g = p.geom;
    plan.op_first.push_back(host_ops.size());
    const int rc = launch_pass(s, p, nullptr, nullptr, &host_ops, &g, oop, job, nullptr, flip, closing);
    plan.geoms.push_back(g);
    plan.passes.push_back(std::move(p));
    return rc;
}

// ---- flush ---------------------------------------------------------------------------------------------
// Decides, for the passes of ONE flush in the order they are pushed, which buffer each reads and writes, and launches them.
// Both sources feed it: the scheduler's sink moves fresh passes in, a replay points at the passes of a cached plan.
//   1. A non-tile pass never changes which buffer holds the state; passes launch in the order pushed.
//   2. No second buffer (spare_buffer() == NULL, asked when the first tile pass arrives: a queue without tile passes allocates
//      nothing) and no PackJob: every pass is launched the moment it is pushed.  Nothing is held back — the GPU works while later
//      passes are still being scheduled.
//   3. With a second buffer every tile pass goes out of place, except that the LAST one does so only if the state is away from
//      its own buffer: the state ends where it started and qsim_device_ptr is stable.  Which tile pass is the last is known only
//      when the next one, or the end, is seen, so the most recent tile pass and the non-tile passes behind it (a group) wait.
//   4. With a PackJob: if the very last pass of the queue is a tile pass that pass_can_pack accepts, given the support the state
//      has once every earlier pass has run, it reads the state from its own buffer and writes the re-layout (job->packed_at says
//      where; the state's own buffers are left holding stale data).  The tile passes before it follow rule 3 among themselves, so
//      the one before it leads home — which is why TWO groups wait then.  Otherwise rule 3 applies to all and packed_at stays NULL.
//   5. After a failed launch the buffers keep their roles.
//   6. With deferred X gates (flip != 0, never together with a PackJob; SchedConfig::defer_flips): the very last pass stores the
//      state at index ^ flip, which only an out-of-place pass can do, and the state must still end at home.  So two groups wait as
//      under rule 4, and the tile pass before the last leads AWAY from home (in place if the state is away already).  flip_ok() says,
//      once every pass has been pushed, whether that works out: the queue ends in a tile pass that has the PACK variant, with a
//      tile pass before it, a second buffer, and every flipped bit inside the support the state then has (a flipped bit outside it
//      would be a qubit in |1> that no zero_mask can express).  If not, the caller drops the flip and pushes the X gates as passes.
//   7. Affine support (QSIM_OPT_AFFINE_SUPPORT; scheduler.h PassRegion): a tile pass may write only the tiles of its region if the
//      next thing to run is a tile pass that tests its input by that region: one of the same schedule, launched plainly.  Every
//      other tile pass is CLOSING and writes the coordinate cube, so that whatever follows (the end of the queue, any other kernel,
//      the re-layout or the flipping pass, the X passes of a dropped flip) finds a state that `support` describes.  Which it is
//      shows only when the next pass is seen: a tile pass that carries a region waits for that even where rule 2 would launch it.
class PassRouter {
  public:
    // rec: the fresh path's recorder for the plan cache, through which the passes moved in are launched (NULL: nothing is recorded)
    PassRouter(qsim_state *s, PackJob *job, PlanRecorder *rec, uint64_t flip = 0)
        : s_(s), job_(job), rec_(rec), home_(s->amps), flip_(job ? 0 : flip), two_(job != nullptr || flip_ != 0), sup_(current_support(s)) {}
    bool flip_ok() const {
        return flip_ != 0 && rc_ == QSIM_OK && pp_ > 0 && held_.size() == 1 && !prev_.empty() && held_[0].p->kclass == QSIM_K_TILE &&
               launch_tile_can_pack(s_->f32, held_[0].tile_geom(), s_->tile_threads) && (flip_ & index_mask(s_->n) & ~sup_) == 0;
    }
    void drop_flip() { flip_ = 0; }
    void push(Pass &&p) { std::unique_ptr<Pass> own(new Pass(std::move(p))); const Pass *at = own.get(); route({at, nullptr, nullptr, std::move(own), nullptr}); }
    void push(const Pass &p, const TileGeom *geom, const TileOp *d_ops, const uint8_t *heads) { route({&p, geom, d_ops, nullptr, heads}); } // of a cached plan: nothing is copied
    int finish() { // the queue has ended
        release(true);
        if (s_->amps != home_) std::swap(s_->amps, s_->spare); // only after a failed launch (rule 5)
        return rc_;
    }

  private:
    struct Item {
        const Pass *p;
        const TileGeom *geom;      // cached plan: the order the tile pass was launched with
        const TileOp *d_ops;       // cached plan: its TileOps on the device
        std::unique_ptr<Pass> own; // a pass the scheduler moved in
        const uint8_t *heads = nullptr; // cached plan: the header bytes of those TileOps (CachedPlan::op_heads)
        const TileGeom &tile_geom() const { return geom ? *geom : p->geom; }
    };
    qsim_state *s_;
    PackJob *job_;
    PlanRecorder *rec_;
    void *const home_;
    uint64_t flip_;  // rule 6
    const bool two_; // two groups wait (rules 4 and 6)
    int rc_ = QSIM_OK;
    int pp_ = -1;  // second buffer available?  -1: not asked yet
    uint64_t sup_; // where the state can be non-zero once every pass pushed so far has run ...
    uint64_t sup_before_last_ = 0; // ... and once every pass but the most recent one has
    std::vector<Item> held_, prev_; // the most recent group; with a PackJob also the one before it

    void launch(Item &it, bool oop, PackJob *pj, uint64_t flip = 0, bool closing = true) {
        if (rc_ != QSIM_OK) return;
        if (it.own && rec_) rc_ = rec_->launch(s_, std::move(*it.own), oop, pj, flip, closing);
        else rc_ = launch_pass(s_, *it.p, it.geom, it.d_ops, nullptr, nullptr, oop, pj, it.heads, flip, closing);
    }
    // oop / pj / flip: of the tile pass at the group's head; next: the tile pass that runs right behind the group, launched plainly
    // (NULL: none, or the re-layout / flipping pass) — rule 7
    void run_group(std::vector<Item> &grp, bool oop, PackJob *pj = nullptr, uint64_t flip = 0, const Item *next = nullptr) {
        const bool closing = grp.size() != 1 || !next || next->p->kclass != QSIM_K_TILE || !next->p->region.on;
        for (size_t i = 0; i < grp.size(); i++) launch(grp[i], i == 0 && oop, i == 0 ? pj : nullptr, i == 0 ? flip : 0, i == 0 ? closing : true);
        grp.clear();
    }
    void route(Item &&it) {
        if (rc_ != QSIM_OK) return;
        const bool tile = it.p->kclass == QSIM_K_TILE;
        sup_before_last_ = sup_;
        sup_ = tile ? sup_ | tile_mask(it.tile_geom()) : ~0ULL; // anything but a tile pass has the zeros written out first
        if (tile && pp_ < 0) pp_ = spare_buffer(s_) != nullptr ? 1 : 0;
        const bool waits = pp_ > 0 || two_ || (tile && it.p->region.on); // rules 3, 4 and 6; rule 7
        if (!waits && held_.empty()) { launch(it, false, nullptr); return; } // rule 2
        if (tile) release(false, &it);
        if (!waits && held_.empty()) { launch(it, false, nullptr); return; } // rule 2 again: the pass that waited under rule 7 has gone
        if (tile || !held_.empty()) held_.push_back(std::move(it));
        else launch(it, false, nullptr); // no tile pass seen yet
    }
    // last = false: a newer tile pass has arrived, so the oldest group held is not the last (rule 3); true: the end of the queue
    // arriving: that newer tile pass
    void release(bool last, const Item *arriving = nullptr) {
        if (!last) {
            if (two_) { // (the group in between is not the last either: it will be launched plainly)
                run_group(prev_, pp_ > 0, nullptr, 0, held_.empty() ? nullptr : &held_[0]);
                prev_.swap(held_);
            } else {
                run_group(held_, pp_ > 0, nullptr, 0, arriving);
            }
            return;
        }
        if (flip_ok()) { // rule 6
            run_group(prev_, s_->amps == home_); // must lead away: the flipping pass is out of place and ends at home
            run_group(held_, true, nullptr, flip_);
            if (rc_ == QSIM_OK) s_->flips_applied++;
            return;
        }
        if (flip_ != 0 && rc_ == QSIM_OK) rc_ = fail(QSIM_ERR_ARG, "internal: deferred flips were neither applied nor dropped");
        const Item *very_last = held_.size() == 1 ? &held_[0] : nullptr; // a tile pass with nothing behind it
        if (job_ && pass_can_pack(s_, very_last ? very_last->p : nullptr, very_last ? very_last->tile_geom() : TileGeom{}, job_, sup_before_last_)) { // rule 4
            run_group(prev_, pp_ > 0 && s_->amps != home_); // must lead home: the packing pass reads the state's own buffer
            if (s_->amps != home_ && rc_ == QSIM_OK) // (cannot happen: the out-of-place passes before came in pairs)
                rc_ = fail(QSIM_ERR_ARG, "internal: state not in its own buffer before the re-layout");
            run_group(held_, false, job_);
        } else {
            run_group(prev_, pp_ > 0, nullptr, 0, held_.empty() ? nullptr : &held_[0]);
            run_group(held_, pp_ > 0 && s_->amps != home_);
        }
    }
};

} // namespace

// How a flush schedules `gates` on a state that has `support` (FlushRule, engine_state.h).  The ONE statement of it: flush_impl runs
// by it, and whatever says beforehand what a flush will do (qsim_support_after, the key choose_schedule files its choice under) asks here.
FlushRule qsim::flush_rule(qsim_state *s, const std::vector<QueuedGate> &gates, uint64_t support, bool for_pack, bool want_key) {
    FlushRule r;
    r.support = support;
    r.cacheable = s->plan_cache && s->fuse >= 3 && s->debug_tile_order == 0 && gates.size() >= 8;
    r.hinted = s->fuse >= 3 && have_sched_hints();
    // only a plain single-state flush defers X gates, and by default only where the planning step chose a schedule that does
    r.defer = !for_pack && (s->defer_flips == 2 || (s->defer_flips == 1 && r.hinted)) && may_defer_flips(s) ? s->defer_flips : 0;
    if (r.cacheable || r.hinted || want_key) {
        r.id = plan_identity(s, gates.size(), support);
        r.id.defer = r.defer;
        r.id.affine = s->affine_support && s->sparse_start ? 1 : 0;
        r.key = gates_key(s, r.id, gates.data(), gates.size());
    }
    return r;
}
SchedConfig FlushRule::config(const qsim_state *s) const {
    SchedConfig cfg = state_sched_config(s, support);
    if (hinted) apply_sched_hint(key, cfg);
    cfg.defer_flips = defer == 2 || (defer == 1 && cfg.defer_flips) ? 1 : 0;
    cfg.affine_support = s->affine_support && s->sparse_start ? 1 : 0; // on wherever a run may start sparse; the schedule is the same either way
    return cfg;
}

// job != NULL: if the LAST pass of the queue is a tile pass that can do it, that pass writes the state re-laid-out (job->packed_at
// says where) and the state's own buffers are left holding stale data; otherwise everything runs as usual and job->packed_at
// stays NULL (the caller then runs the pack kernel).
int qsim::flush_impl(qsim_state *s, PackJob *job) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    QSIM_TRY(await_buffer(s)); // (everything that looks at the buffer flushes first: the one place to wait for qsim_create_async)
    if (s->queue.empty()) return QSIM_OK;
    if (s->zero_ket_pending && s->zero_ket_amp == 0.0) { // the all-zero vector (a shard that holds nothing yet): every gate maps it to itself
        s->queue.clear();
        return QSIM_OK;
    }
    if (s->tile_bits - s->tile_low_bits < 2 || s->tile_bits - s->tile_low_bits > kMaxTileHigh)
        return fail(QSIM_ERR_ARG, "tile_bits - tile_low_bits must be in 2..%d", kMaxTileHigh);
    HIP_TRY(hipSetDevice(s->device));
    FlushRule rule = flush_rule(s, s->queue, current_support(s), job != nullptr);
    const bool cacheable = rule.cacheable;
    const uint64_t key = rule.key, epoch = wisdom_epoch();
    // The flips the router could not hand to the last tile pass (PassRouter rule 6) run as X gates in passes of their own,
    // scheduled the ordinary way and pushed behind the others: right, at the price of one more pass, and counted.
    auto settle_flips = [&](PassRouter &router, uint64_t flip) {
        if (flip == 0 || router.flip_ok()) return;
        router.drop_flip();
        s->flip_fallbacks++;
        static const cd kX[4] = {cd(0, 0), cd(1, 0), cd(1, 0), cd(0, 0)};
        Scheduler xs(state_sched_config(s, ~0ULL)); // (dense: the gates behind these X gates may have made any support)
        for (int q = 0; q < s->n; q++)
            if (flip >> q & 1ULL) xs.add_1q(kX, q);
        xs.finish([&](Pass &&p) { router.push(std::move(p)); });
    };
    if (const CachedPlan *pl = cacheable ? find_plan(s, key, epoch, rule.id) : nullptr) { // replay: no scheduling, no block preparation, no H2D copy
        s->queue.clear();
        PassRouter router(s, job, nullptr, pl->flip);
        for (size_t i = 0; i < pl->passes.size(); i++) {
            const bool tile = pl->passes[i].kclass == QSIM_K_TILE;
            router.push(pl->passes[i], tile ? &pl->geoms[i] : nullptr, tile ? pl->d_ops + pl->op_first[i] : nullptr,
                        tile ? pl->op_heads.data() + kHeadBytes * pl->op_first[i] : nullptr);
        }
        settle_flips(router, pl->flip); // (a plan is recorded with the flip its last pass took, so this finds nothing to do)
        return router.finish();
    }
    Scheduler sched(rule.config(s));
    feed(sched, s->queue);
    const uint64_t flip = sched.residual_flips(); // known before the first pass is built
    PlanRecorder rec;
    if (cacheable) {
        rec.plan.id = std::move(rule.id);
        rec.plan.id.gates = std::move(s->queue); // the plan remembers what it was built from
    }
    s->queue.clear();
    // passes are launched as they are scheduled, as far as the routing allows (PassRouter, rules 2 and 3)
    PassRouter router(s, job, cacheable ? &rec : nullptr, flip);
    sched.finish([&](Pass &&p) { router.push(std::move(p)); });
    rec.plan.flip = router.flip_ok() ? flip : 0;
    settle_flips(router, flip);
    const int rc = router.finish();
    return rc != QSIM_OK || !cacheable ? rc : keep_plan(s, rec, key, epoch);
}

bool qsim::may_defer_flips(qsim_state *s) {
    if (s->defer_flips == 0 || s->fuse < 3 || s->f32 || !s->owns) return false;
    if (!s->alloc_done.load()) return false; // qsim_create_async is still allocating the first buffer: the second cannot be asked for beside it (every flush has joined that)
    TileGeom g{};
    g.tile_bits = std::min(s->tile_bits, s->n);
    if (!launch_tile_can_pack(false, g, s->tile_threads)) return false;
    return spare_buffer(s) != nullptr && s->owns_spare;
}

int qsim::written(qsim_state *s, bool keep_partial) {
    const int rc = qsim_flush(s);
    if (rc || (keep_partial && !s->zero_ket_pending && s->partial)) return rc;
    return materialize_zero_ket(s); // nothing consumed the pending |0...0>, or the zeros outside the support: write them now
}
int qsim::settle(qsim_state *s, bool keep_partial) {
    QSIM_TRY(written(s, keep_partial));
    HIP_TRY(hipSetDevice(s->device)); // a cluster drives several devices from one thread
    return QSIM_OK;
}

extern "C" int qsim_flush(qsim_state *s) { return flush_impl(s, nullptr); }

extern "C" int qsim_plan_cache_stats(const qsim_state *s, uint64_t *plans, uint64_t *replays, uint64_t *key_collisions) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    if (plans) *plans = s->plans.size();
    if (replays) *replays = s->plan_hits;
    if (key_collisions) *key_collisions = s->plan_key_collisions;
    return QSIM_OK;
}

extern "C" int qsim_deferred_flip_stats(const qsim_state *s, uint64_t *applied, uint64_t *fallbacks) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    if (applied) *applied = s->flips_applied;
    if (fallbacks) *fallbacks = s->flip_fallbacks;
    return QSIM_OK;
}

extern "C" int qsim_sync(qsim_state *s) {
    QSIM_TRY(written(s));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return QSIM_OK;
}
