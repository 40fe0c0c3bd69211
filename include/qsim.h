/*
 * qsim.h — C ABI of libqsim.so, the MI355X-native state-vector engine.
 *
 * Plain C: opaque handles, pointers and sizes only.  Every entry point names the reference interface
 * it stands in for (file:line into RiccardoFiorentini/GPU_quantum_simulator).  The reference has no
 * plugin/FFI layer: its drop-in surface is the CLI of quantum_simulator.c plus the three C functions
 * declared at quantum_simulator.c:25-27, which live in qsim_legacy.h.  This header is the handle API
 * those are built on — the state vector stays in HBM between gates.
 *
 * Conventions (quantum_simulator.c:83): qubit k is bit k of the amplitude index, q[0] = LSB.
 * Amplitudes are fp64 complex, array-of-structs (re, im), 16 bytes each, exactly the memory layout of
 * C99 `double _Complex` (quantum_simulator.c:35,168).  Matrices are row-major, (re, im) interleaved,
 * and mean the standard U·v (NOT the transposed product of quantum_simulator.c:88-89; the legacy
 * wrapper transposes for you).
 *
 * All functions return QSIM_OK (0) or a QSIM_ERR_* code; qsim_last_error() gives the message.
 * The library never falls back to a CPU path: without a usable HIP device qsim_create fails.
 */
#ifndef QSIM_H
#define QSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qsim_state qsim_state;     /* one state vector (or one shard of it) resident on one GPU */
typedef struct qsim_circuit qsim_circuit; /* parsed gate list, host memory */

enum {
    QSIM_OK = 0,
    QSIM_ERR_ARG = 1,    /* bad argument (NULL handle, qubit out of range, ...) */
    QSIM_ERR_ALLOC = 2,  /* host or device allocation failed  ("Malloc error", quantum_simulator.c:170) */
    QSIM_ERR_DEVICE = 3, /* HIP runtime error / no device */
    QSIM_ERR_OPEN = 4,   /* cannot open circuit file          (quantum_simulator.c:128-131) */
    QSIM_ERR_PARSE = 5   /* unknown token / malformed circuit (quantum_simulator.c:212-223) */
};

/* Gate kinds in a qsim_circuit. */
enum { QSIM_GATE_U1 = 1, QSIM_GATE_CX = 2, QSIM_GATE_U2 = 3, QSIM_GATE_U3 = 4, QSIM_GATE_U4 = 5, QSIM_GATE_U5 = 6, QSIM_GATE_U6 = 7, QSIM_GATE_U7 = 8, QSIM_GATE_U8 = 9 /* U3..U8: scheduler output only */ };

/* Options for qsim_set_option. */
enum {
    /* How adjacent gates are merged before launch:
     *   0  one launch per gate                      (quantum_simulator_naive.cu:163-189)
     *   1  per-qubit 2x2 accumulation, flush at CX  (quantum_simulator_preproces.cu:215-269)
     *   2  pair clusters folded into one 4x4        (quantum_simulator_4x4.cu:327-501)
     *   3  level 2 + cache-blocked passes: several clusters applied to an LDS-resident tile per
     *      launch, op list read from device memory  (idea of quantum_simulator_preproces_constant.cu:169-178,
     *      done with a full grid)                   [default]                                        */
    QSIM_OPT_FUSE = 1,
    QSIM_OPT_PROFILE = 2,      /* 1: bracket every launch with HIP events on the engine's stream; 2: also record each tile pass's block forms (qsim_launch_log_blocks) */
    QSIM_OPT_TILE_BITS = 3,    /* log2 amplitudes per LDS tile for level 3 (8..13 in either precision, default 12 = 64 KiB of fp64) */
    QSIM_OPT_TILE_LOW_BITS = 4,/* contiguous low index bits always inside a tile (2..6, default 3 -> 128-B runs, 9 free high-qubit slots) */
    QSIM_OPT_MAX_PENDING = 5,  /* queued gates that force a flush (default 1<<16) */
    QSIM_OPT_TILE_MAX_OPS = 6, /* upper bound on fused blocks per tile pass (default 32) */
    QSIM_OPT_GRID_CAP = 7,     /* 0: one workgroup per work tile; >0: at most that many workgroups (grid-stride loop) */
    QSIM_OPT_TILE_PAD_FROM = 9,/* first index bit used to fill unused high slots of a tile (default 10) */
    QSIM_OPT_TILE_THREADS = 8, /* threads per tile workgroup: 0 auto (256 below 2^12 amplitudes, else 512), 256, 512, 1024 */
    /* 10 and 11 were measurement aids; they are retired and rejected like any unknown option */
    QSIM_OPT_PLAN_CACHE = 13,  /* default 1: the plans of the last few flushed gate queues are kept (passes, bit orders, blocks on the
                                * device); a queue with the same gates is replayed without scheduling or uploads.  0 = plan anew */
    QSIM_OPT_PINGPONG = 14,    /* tile passes out of place: each reads the state from one buffer and writes it to a second one, and the
                                * two swap (an even number of times per flush: the state is back in its own buffer afterwards).  The
                                * same bytes move ~5 % faster than in place at n = 30.  0 never, 1 (default) for states of >= 8 GiB
                                * when the second buffer fits (allocated on first use, or lent with qsim_set_spare_buffer), 2 always */
    QSIM_OPT_AFFINE_SUPPORT = 18,/* default 1: inside one flush, tile passes over a partially written state (QSIM_OPT_SPARSE_START) visit only
                                 * the tiles of the affine subspace of index space the support lies in — X translates it, CX maps it
                                 * linearly, only a mixing gate adds a direction — instead of the whole cube over the qubits touched.
                                 * Schedules are the same either way; 0: every launch is what it was without the option. */
    QSIM_OPT_SPARSE_START = 15,/* default 1: after a reset the state is zero wherever a qubit no pass has mixed yet is 1, and the tile
                                * passes only visit the rest: the first pass of a circuit writes one tile, the second a few hundred,
                                * the full sweeps start when every qubit has been inside a tile (memory outside that support is
                                * written as zeros the moment anything else looks at the buffer).  0 = every pass sweeps the register */
    QSIM_OPT_DEBUG_PLAN_KEY = 16,/* test aid, default 0: k != 0 = every flushed queue gets the plan-cache key k, i.e. all circuits collide;
                                  * results must not change — a cached plan is only replayed after its gate list, options and
                                  * support have been compared with the queue's (qsim_plan_cache_stats counts the collisions) */
    QSIM_OPT_DEFER_FLIPS = 17, /* X gates as an index flip in the stores of a flush's last tile pass instead of scheduled gates: an X moves
                                * past every later gate exactly (the gate's matrix with rows and columns permuted), so the X gates of a
                                * queue, and the X factor of every anti-diagonal 2x2, collapse into one mask at its end and force no
                                * qubit into any tile.  Only a plain flush of an fp64 state in the default tile shape (2^12 amplitudes,
                                * 512 threads) whose passes run out of place between two buffers of its own can do that; every other
                                * flush schedules the X gates as before.  0 never, 1 (default) where the planning step chose such a
                                * schedule for the circuit, 2 wherever possible.  qsim_deferred_flip_stats counts */
    QSIM_OPT_DEBUG_TILE_ORDER = 12,/* measurement aid, default 0: k > 0 = every tile pass walks its high tile bits in a pseudo-random
                                  * order seeded by k (results are unchanged: the order only decides which bits lanes, waves and
                                  * registers walk) */
};

/* Kernel classes reported by qsim_get_stats. */
enum {
    QSIM_K_INIT = 0,
    QSIM_K_GATE1 = 1,  /* dense 2x2, target bit >= 6: two coalesced streams            */
    QSIM_K_GATE1_LO = 2,/* dense 2x2, target bit < 6: in-wave shuffle butterfly         */
    QSIM_K_PHASE = 3,  /* diag(1, lambda): touches the bit=1 half only                 */
    QSIM_K_CX = 4,     /* swap on the control=1 half                                   */
    QSIM_K_GATE2 = 5,  /* dense 4x4 (any bit positions)                                */
    QSIM_K_TILE = 6,   /* cache-blocked multi-op pass                                  */
    QSIM_K_PACK = 7,   /* shard re-layout before a global<->local qubit exchange       */
    QSIM_K_COUNT = 8
};

typedef struct {
    uint64_t gates;                     /* gate statements accepted (pre-fusion)                     */
    uint64_t launches;                  /* kernels launched                                          */
    double algorithmic_bytes;           /* sum over launches of the bytes the pass must move         */
    uint64_t k_launches[QSIM_K_COUNT];
    double k_bytes[QSIM_K_COUNT];       /* algorithmic bytes per class                               */
    double k_ms[QSIM_K_COUNT];          /* HIP-event time per class (QSIM_OPT_PROFILE=1), else 0     */
} qsim_stats;

/* ---- device / lifecycle -------------------------------------------------------------------------- */
int qsim_device_count(void);
/* Creates the HIP context of `device` (first-touch cost of the runtime, a few hundred ms per process).  The C host
 * calls it before starting its clock: it is process start-up, not part of the gate path the reference times. */
int qsim_device_init(int device);
const char *qsim_last_error(void);

/* Allocates 2^num_q amplitudes on `device` and sets |0...0>.  Replaces the malloc + init loop of the
 * `qubit` statement (quantum_simulator.c:168-177) and init_state_vector (quantum_simulator_naive.cu:64-70). */
int qsim_create(qsim_state **out, int num_q, int device);
/* Same, with the amplitudes held as fp32 complex (8 bytes each): the precision of the reference's CUDA variants
 * (`cuFloatComplex`, quantum_simulator_naive.cu:38,64-70).  Half the HBM bytes per pass and one more qubit per GPU;
 * every entry point keeps its double-typed interface (matrices are rounded once when a pass is built, qsim_read /
 * qsim_write convert), sums (norm, sampling) still accumulate in fp64.  Not the parity configuration: results agree
 * with quantum_simulator.c to fp32 rounding (~1e-6 per amplitude), not to 1e-10.  Clusters are fp64 only. */
int qsim_create_f32(qsim_state **out, int num_q, int device);
/* Same as qsim_create / qsim_create_f32 (precision_bits 64 / 32) with the amplitude buffer allocated on a helper thread: the call
 * returns at once — hipMalloc of a 16 GiB state takes 0.04-0.25 s, the largest single item of a cold run
 * (quantum_simulator.c:168-177 has malloc in the same place) — so that parsing, options, gate queueing and the schedule choice
 * run beside it.  The first call that needs the buffer waits for it; an allocation failure surfaces there as QSIM_ERR_ALLOC. */
int qsim_create_async(qsim_state **out, int num_q, int device, int precision_bits);
int qsim_precision_bits(const qsim_state *s); /* 64 or 32; -1 for NULL */
/* Same, on caller-owned device memory of 16<<num_q bytes (e.g. a torch tensor's storage). */
int qsim_create_external(qsim_state **out, int num_q, int device, void *device_amps);
void qsim_destroy(qsim_state *s);
int qsim_reset(qsim_state *s); /* back to |0...0>; drops queued gates.  Lazy: written by the first pass that can
                                 * generate it in LDS, or by the init kernel when anything else comes first */
/* Same for one shard of a larger register: holds_index0 = 0 gives the all-zero vector (the shard does not contain
 * basis index 0). */
int qsim_reset_shard(qsim_state *s, int holds_index0);
int qsim_num_qubits(const qsim_state *s);
int qsim_set_option(qsim_state *s, int option, long value);
long qsim_get_option(const qsim_state *s, int option);

/* ---- gates: queued in program order, merged and launched at flush ---------------------------------- */
/* execute_single_qubit_gate (quantum_simulator.c:81-92), kernel_gate (quantum_simulator_naive.cu:72-95).
 * U: 4 complex, row-major, standard U·v. */
int qsim_apply_1q(qsim_state *s, const double *U, int target);
/* execute_cnot (quantum_simulator.c:94-106), kernel_cnot (quantum_simulator_naive.cu:97-122). */
int qsim_apply_cx(qsim_state *s, int control, int target);
/* kernel_gate_4 (quantum_simulator_4x4.cu:109-146): U is 16 complex, row/col index = (bit q_hi, bit q_lo). */
int qsim_apply_2q(qsim_state *s, const double *U, int q_hi, int q_lo);
int qsim_flush(qsim_state *s); /* schedule + launch everything queued; returns without waiting */
/* QSIM_OPT_PLAN_CACHE bookkeeping: plans held, flushes served by replaying one, and 64-bit key matches that were REJECTED because
 * the cached plan's gate list / options / support differed from the queue's (the key only finds candidates). */
int qsim_plan_cache_stats(const qsim_state *s, uint64_t *plans, uint64_t *replays, uint64_t *key_collisions);
int qsim_sync(qsim_state *s);  /* flush, then wait for the stream */
/* QSIM_OPT_DEFER_FLIPS: *applied = flushes whose last tile pass stored the state with the deferred X gates' index flip; *fallbacks =
 * flushes that were scheduled with deferred X gates but could not end that way (no tile pass at the end or none before it, a
 * flipped qubit outside the state's support) and ran the X gates in a pass of their own.  Since the state was created. */
int qsim_deferred_flip_stats(const qsim_state *s, uint64_t *applied, uint64_t *fallbacks);

/* ---- amplitudes in / out (the reference's final cudaMemcpy D2H, quantum_simulator_naive.cu:193-194) -- */
int qsim_read(qsim_state *s, uint64_t first, uint64_t count, double *out_re_im);
int qsim_write(qsim_state *s, uint64_t first, uint64_t count, const double *in_re_im);
int qsim_norm2(qsim_state *s, double *out); /* sum |a|^2 computed on the device: the identity string of qsim_expect_paulis below, one
                                             * read-only sweep, fp64 sums in a fixed order (equal calls return equal bits) */
/* ---- expectation values of Pauli strings, computed on the device (new: the reference has no observables) ----
 * A string on the register is two masks: bit q of x_mask set where it has X or Y on qubit q, bit q of z_mask where it has Z or Y
 * (both: Y).  out[t] = <psi|P_t|psi>, a real number, for num_terms strings; coefficients of a Hamiltonian are the caller's.
 * Launches queued gates first; does not modify the state.  Terms are grouped by x_mask: all strings with one x_mask share the
 * loads and the pair products, so each group costs ceil(size / K) read-only sweeps of the state, K = qsim_pauli_terms_per_sweep().
 * The sums are fp64 in both precisions and are formed in a fixed order: equal calls return equal bits.  One device-to-host
 * copy and one stream synchronise per 128 sweeps.  The identity (x = z = 0) is legal and gives the squared norm;
 * num_terms == 0 succeeds and writes nothing.  QSIM_ERR_ARG: NULL arguments with num_terms > 0, a mask bit at or above the
 * register's qubit count, a negative num_terms. */
int qsim_expect_paulis(qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, double *out);
/* Host only, no device: how many sweeps the call above makes for these terms. */
int qsim_pauli_sweeps(const uint64_t *x_masks, long num_terms, long *sweeps);
int qsim_pauli_terms_per_sweep(void); /* K: 32 ("Expectation values": the measured choice among 8, 16, 32) */
/* ---- Pauli-string rotations exp(-i theta/2 P), applied on the device (new: the reference has neither observables nor rotations) ----
 * The other half of qsim_expect_paulis: strings are the same two masks.  state <- prod_t exp(-i thetas[t]/2 P_t) state, t = 0
 * first, in the caller's order (nothing is reordered, whether or not terms commute).  Convention: exp(-i theta/2 Z_q) =
 * diag(e^(-i theta/2), e^(+i theta/2)) on qubit q, which is e^(-i theta/2) times the gate table's rz(theta) = diag(1, e^(i theta))
 * (qsim_gate_matrix; quantum_simulator.c:184-211): the table drops the global phase, a rotation keeps it.  The identity string
 * (x = z = 0) is that global phase e^(-i theta/2) alone.
 * Routing: a term that is X or Y on ONE qubit is queued as its 2x2 (qsim_apply_1q: it fuses with neighbouring gates, no sweep).
 * Every other term — single-qubit Z terms included — goes to an in-place sweep of the state (one read, one write, for a string of
 * any weight), launched after the queued gates; a maximal run of consecutive sweep terms with equal x_mask shares sweeps, K =
 * qsim_pauli_rotations_per_sweep() terms each, applied in registers in order (all-Z terms, x_mask = 0, are one such run).
 * cos and sin of theta/2 are formed on the host in fp64 and rounded once to the state's precision, as gate matrices are.
 * Returns without waiting: the sweeps are on qsim_stream(); no device allocation, no host synchronisation.  A sweep's grid is as
 * many workgroups as are resident at once, each walking a grid-stride loop; QSIM_OPT_GRID_CAP > 0 caps it instead, as for every kernel.  Every amplitude is
 * written by one thread: equal calls give equal bits.  Sweeps are NOT counted in the qsim_stats record: they have no QSIM_K_* class of their own, the
 * struct keeps its layout; the queued 2x2s are, as gates.  A shard that holds nothing (qsim_holds_nothing) stays untouched.
 * num_terms == 0 succeeds and does nothing.  QSIM_ERR_ARG, with the state unchanged: a NULL state, NULL arrays with num_terms > 0,
 * a negative num_terms, a mask bit at or above the register's qubit count, a non-finite theta. */
int qsim_apply_pauli_rotations(qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, const double *thetas, long num_terms);
/* Host only, no device: what the call above does with these terms — sweeps launched and terms queued as 2x2 gates. */
int qsim_pauli_rotation_plan(const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, long *sweeps, long *queued_as_gates);
int qsim_pauli_rotations_per_sweep(void); /* K: 32, the one-bit-per-term masks' limit; an unmeasured default ("Pauli rotations") */
/* ---- controlled Pauli rotations: "... if these qubits are 1" (new) ----
 * qsim_apply_pauli_rotations with a control mask per term: term t maps the state to [(1 - Pi_t) + Pi_t exp(-i thetas[t]/2 P_t)] state,
 * Pi_t the projector on "every qubit of c_masks[t] is 1"; angle convention and kept global phase as above, so the identity string
 * (x = z = 0) under controls is the multi-controlled phase e^(-i theta/2) on the control subspace (theta = -2 phi: diag(1, ..., 1,
 * e^(i phi)) on the control qubits; phi = pi: a multi-controlled Z).  Terms are applied in the caller's order.  c_masks == NULL: no
 * controls anywhere; a term with c_masks[t] == 0 takes exactly the path qsim_apply_pauli_rotations gives it, and a call without
 * any control leaves the bits that call leaves.
 * Routing of a term WITH controls: one control and X or Y on ONE qubit is queued as its 4x4 (qsim_apply_2q: it fuses like a cx, no
 * sweep).  Every other controlled term — controlled single-qubit Z terms and the controlled identity included — goes to a
 * controlled sweep, launched after the queued gates: the 2x2 of the uncontrolled sweep on the same pairs {j, j ^ x}, but only on
 * the 2^(n-c) indices whose c control bits are 1, so it reads and writes 2^-c of the state.  A maximal run of consecutive sweep
 * terms with equal x_mask AND equal control mask shares sweeps, qsim_pauli_rotations_per_sweep() terms each; a change of control
 * mask ends a run as a change of x_mask does.  Controlled sweeps count in qsim_pauli_rotation_sweeps_launched().
 * Otherwise as qsim_apply_pauli_rotations: returns without waiting, no device allocation, no host synchronisation,
 * QSIM_OPT_GRID_CAP applies, every amplitude is written by one thread (equal calls give equal bits; an amplitude inside the
 * control subspace gets the bits the uncontrolled sweep of the same terms gives it), a shard that holds nothing stays untouched,
 * num_terms == 0 does nothing, a lazily held |0...0> or a partial state is settled first and the support is dense afterwards.
 * QSIM_ERR_ARG, with the state unchanged: everything qsim_apply_pauli_rotations refuses, a control bit at or above the register's
 * qubit count, and a control mask that overlaps the term's x_mask | z_mask (a control qubit carries a Pauli factor).
 * Gradients through controlled terms: qsim_controlled_pauli_gradient below.
 * Out of scope: controls on clusters or shards (no qsim_cluster_* counterpart), controlled terms in product formulas
 * (Simulator.evolve), and a QASM spelling — the parser's grammar is the reference's. */
int qsim_apply_controlled_pauli_rotations(qsim_state *s, const uint64_t *c_masks, const uint64_t *x_masks, const uint64_t *z_masks,
                                          const double *thetas, long num_terms);
/* Host only, no device: what the call above does with these terms on a register of num_q qubits held in precision_bits (64 or 32)
 * — sweeps launched, terms queued as gates (2x2 and 4x4 together), and units_visited: the sum over the sweeps of the 16-byte units
 * (one fp64 amplitude, two fp32 amplitudes) the sweep's loop visits, from the geometry function its launcher uses.  Without
 * controls the first two are qsim_pauli_rotation_plan's.  QSIM_ERR_ARG as above, and for num_q outside [0, 40], precision_bits
 * other than 64 or 32, a NULL result pointer. */
int qsim_controlled_rotation_plan(const uint64_t *c_masks, const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, int num_q,
                                  int precision_bits, long *sweeps, long *queued_as_gates, uint64_t *units_visited);
/* ---- adjoint-mode gradients of <H> for circuits of Pauli rotations, on the device (new) ----
 * E = <psi_K|H|psi_K> and grad[k] = dE/dtheta_k for psi_K = prod_k exp(-i thetas[k]/2 P_k) |state>, H = sum_t coeffs[t] Q_t (real
 * coefficients): all num_rot derivatives from one forward pass, one application of H and one backward pass, instead of the two
 * circuit executions per parameter of the shift rule.  With |lambda_K> = H|psi_K> and |lambda_(k-1)> = U_k^+ |lambda_k>,
 * dE/dtheta_k = Im <lambda_k|P_k|psi_k>.
 * Forward: qsim_apply_pauli_rotations (its routing, single X/Y through the gate queue).  Then lambda = H psi (one out-of-place sweep
 * per piece of an x_mask group of H, qsim_pauli_terms_per_sweep() terms each), energy = Re <lambda|psi> (one paired sweep), then the
 * backward sweeps: maximal runs of consecutive equal x_mask, cut into pieces of qsim_pauli_rotations_per_sweep(), last run first; a
 * sweep reads and writes psi and lambda once and differentiates AND undoes its terms in registers, from the last to the first,
 * whether or not they commute.  In the backward pass EVERY term goes through a sweep, single X/Y and the identity included (the
 * identity's derivative is 0 up to rounding: a global phase).
 * lambda lives in the state's spare buffer when it has one (it is idle outside a flush), otherwise in a buffer of the state's own
 * that is allocated on first use and freed by qsim_destroy — whatever QSIM_OPT_PINGPONG says, and for external states too.
 * QSIM_ERR_ALLOC when that fails, with the state untouched.  The sums are fp64 in both precisions and are added in a fixed order:
 * equal calls return equal bits, and QSIM_OPT_GRID_CAP does not apply to the backward sweeps (it would change the order).  The
 * results of up to 128 sweeps travel in one device-to-host copy; the call waits for its results.
 * On return the state holds what it held before the call, to the rounding of 2 num_rot rotations.  energy or grad may be NULL.
 * num_rot == 0: the energy alone.  A shard that holds nothing (qsim_holds_nothing): energy 0, grad zeros, no sweep.
 * QSIM_ERR_ARG, with the state unchanged: a NULL state, NULL arrays with a positive count, a negative count, a mask bit at or above
 * the register's qubit count, a non-finite theta or coefficient.
 * Single states only, fp64 and fp32: there is NO qsim_cluster_* counterpart (a sharded lambda needs a second exchange scratch). */
int qsim_pauli_gradient(qsim_state *s, const uint64_t *rot_x, const uint64_t *rot_z, const double *thetas, long num_rot,
                        const uint64_t *ham_x, const uint64_t *ham_z, const double *coeffs, long num_ham, double *energy, double *grad);
/* dst (device, 2^n amplitudes of the state's precision, not the state's own buffers) = sum_t coeffs[t] Q_t |state>; on qsim_stream(),
 * not waited for.  num_terms == 0 writes zeros.  QSIM_ERR_ARG as above, and for dst_device NULL or equal to the state's buffer or
 * its spare buffer. */
int qsim_pauli_sum_into(qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, const double *coeffs, long num_terms, void *dst_device);
/* Host only: sweeps the gradient call makes after its forward pass. */
int qsim_pauli_gradient_plan(const uint64_t *rot_x, long num_rot, const uint64_t *ham_x, long num_ham, long *adjoint_sweeps, long *sum_sweeps);
/* ---- adjoint-mode gradients through controlled Pauli rotations (new) ----
 * qsim_pauli_gradient with a control mask per rotation: U_k = (1 - Pi_k) + Pi_k exp(-i thetas[k]/2 P_k), Pi_k the projector on
 * "every qubit of rot_c[k] is 1" (qsim_apply_controlled_pauli_rotations' terms).  dU_k/dtheta_k = -(i/2) Pi_k P_k U_k, so
 * grad[k] = Im <lambda_k| Pi_k P_k |psi_k>: the pair sums of qsim_pauli_gradient taken inside the control subspace only.  The generator
 * Pi P / 2 has the eigenvalues 0 and +-1/2, so the two-term shift rule gives a WRONG derivative for a controlled term and the exact
 * rule needs four circuit executions per parameter; this call needs one forward and one backward pass for all of them.
 * rot_c == NULL: no controls anywhere — qsim_pauli_gradient is this call with NULL, and a call without any control returns the bits
 * that call returns for energy, gradient and state.
 * Forward: the routing of qsim_apply_controlled_pauli_rotations (one control on a single X or Y through the gate queue as its 4x4).
 * Backward: EVERY term goes through a sweep; the pieces are maximal runs of consecutive equal x_mask AND equal control mask, cut into
 * qsim_pauli_rotations_per_sweep(), last first.  A piece without controls is qsim_pauli_gradient's sweep; a piece with c controls
 * reads and writes the 2^-c of psi and of lambda that the subspace holds and leaves every other amplitude's bits alone.  Both count in
 * qsim_pauli_adjoint_sweeps_launched().
 * Everything else is as qsim_pauli_gradient promises: where lambda lives, allocation before the state is touched (QSIM_ERR_ALLOC),
 * fp64 sums in a fixed order (equal calls return equal bits, QSIM_OPT_GRID_CAP does not apply), 128 result rows per copy, the state
 * left as found to rounding, energy or grad may be NULL, num_rot == 0 gives the energy alone, a shard that holds nothing gives energy
 * 0, zero gradient and no sweep, a lazily held |0...0> is settled first.
 * QSIM_ERR_ARG, with the state unchanged: whatever qsim_pauli_gradient or qsim_apply_controlled_pauli_rotations refuses — a control bit
 * at or above the register's qubit count and a control mask that overlaps the term's x_mask | z_mask included.
 * Single states only, fp64 and fp32. */
int qsim_controlled_pauli_gradient(qsim_state *s, const uint64_t *rot_c, const uint64_t *rot_x, const uint64_t *rot_z, const double *thetas,
                                   long num_rot, const uint64_t *ham_x, const uint64_t *ham_z, const double *coeffs, long num_ham, double *energy,
                                   double *grad);
/* Host only, no device: the sweeps the call above makes after its forward pass on a register of num_q qubits held in precision_bits
 * (64 or 32), and units_visited: the sum over the BACKWARD sweeps of the 16-byte units the sweep's loop visits, from the geometry
 * function its launcher uses — multiplied by nothing: one unit index addresses psi and lambda.  Without controls (rot_c NULL or all
 * zero) the first two are qsim_pauli_gradient_plan's.  The plan knows no z_mask: a control that meets the term's x_mask is refused
 * here, one that meets its z_mask by the call itself.  Otherwise QSIM_ERR_ARG as for qsim_controlled_rotation_plan. */
int qsim_controlled_gradient_plan(const uint64_t *rot_c, const uint64_t *rot_x, long num_rot, const uint64_t *ham_x, long num_ham, int num_q,
                                  int precision_bits, long *adjoint_sweeps, long *sum_sweeps, uint64_t *units_visited);
/* ---- state algebra: calls that take more than one state (new) ----
 * All states of a call have the same qubit count, the same precision and the same device, else QSIM_ERR_ARG.  Every state involved is
 * settled first: queued gates launched, a lazily held |0...0> or a partly written support written out; a shard that holds nothing
 * counts as zeros.  A destination that is overwritten without being read gets no zeros first (its queued gates are dropped with
 * it); afterwards it is an ordinary dense state.  The work runs on the destination's stream (the inner product: on a's), after an
 * event recorded on every source's stream, and every source's stream waits for an event recorded behind it: a gate queued on a
 * source afterwards cannot overtake the read. */
/* dst <- src, bit for bit.  dst != src.  Not waited for. */
int qsim_copy_state(qsim_state *dst, qsim_state *src);
/* <a|b> = sum_i conj(a_i) b_i: one read-only sweep over both buffers, real and imaginary part from the same loads, fp64 sums in a
 * fixed order (equal calls return equal bits).  a == b is allowed and gives (the squared norm, 0).  Waits for its result. */
int qsim_inner(qsim_state *a, qsim_state *b, double *re, double *im);
/* dst <- d dst + a p + b q, complex coefficients as (re, im); q (and b) may be NULL: no third state.  *norm2 (may be NULL) = the squared
 * norm of dst as stored, from the same sweep: what the norm call would return afterwards up to the order of summation, formed in a
 * fixed order whatever QSIM_OPT_GRID_CAP says.  The coefficients are rounded once to the states' precision and the multiply-adds run
 * in it.  d == 0: dst is NOT read — it may hold anything, NaN included; with q == NULL that is the scaled copy dst <- a p.  Waits for
 * the device only when norm2 is asked for.  QSIM_ERR_ARG, nothing touched: dst is p or q, a NULL dst, d, p or a, a non-finite
 * coefficient, states that differ in shape. */
int qsim_combine(qsim_state *dst, const double d[2], qsim_state *p, const double a[2], qsim_state *q, const double b[2], double *norm2);
/* ---- the lowest eigenvalue of a Pauli-sum Hamiltonian by Lanczos iteration, on the device (new) ----
 * H = sum_t coeffs[t] Q_t as for the gradient call.  From v_0 = state / |state|, step j = 0, 1, ...: w = H v_j, alpha_j = Re <v_j|w>,
 * w <- w - alpha_j v_j - beta_(j-1) v_(j-1), beta_j = |w| (from the same sweep), v_(j+1) = w / beta_j — no reorthogonalisation, which
 * the LOWEST Ritz value does not need (interior eigenvalues are not offered for that reason).  After every step the host solves the
 * tridiagonal of the alphas and betas for its lowest eigenvalue theta and unit eigenvector t; beta_j |t_last| estimates the residual
 * |H y - theta y| of the unit Ritz vector y.  The call stops when that is <= tol (an absolute bound), at max_steps, or when
 * beta_j <= 64 eps sum_t |coeffs[t]| (eps = 2^-53 or 2^-24 with the precision): the Krylov space of the start vector is exhausted.
 * All three return QSIM_OK with *steps = steps done, *energy = theta and alphas[0..steps), betas[0..steps) filled (NULL, or max_steps
 * entries each).  want_vector == 0: *residual = the estimate, and the state keeps the bits it had (its buffer is only read).
 * want_vector != 0: a second pass re-runs the recurrence with the recorded alphas and betas and accumulates y = sum_j t_j v_j in the
 * state's own buffer; one more application of H then MEASURES *residual = |H y - theta y|, and the state ends as y at unit norm.
 * Cost of a step: the sweeps of one H application (3 G - 1 state volumes for G sweeps), one paired read-only sweep for alpha (2) and
 * the update (4); two small host synchronisations (alpha, then beta).  Memory: three work buffers of the state's size — the idle spare
 * buffer and the gradient's lambda buffer where the state has them, the rest allocated before anything is touched (QSIM_ERR_ALLOC
 * leaves the state untouched) and freed before returning.  Sums are fp64 in a fixed order: equal calls return equal bits.
 * num_ham == 0 is H = 0: one step, energy 0.  QSIM_ERR_ARG, with the state unchanged: everything the Pauli-sum call refuses,
 * max_steps < 1, a negative or non-finite tol, a state of norm zero or a shard that holds nothing.
 * Single states only, fp64 and fp32: there is NO cluster counterpart. */
int qsim_lanczos_ground(qsim_state *s, const uint64_t *ham_x, const uint64_t *ham_z, const double *coeffs, long num_ham, int max_steps, double tol,
                        int want_vector, double *energy, double *residual, int *steps, double *alphas, double *betas);
/* Host only: the lowest eigenvalue *theta of the symmetric tridiagonal with diagonal alphas[0..m) and off-diagonal betas[0..m-1)
 * (bisection), and its unit eigenvector vec[0..m) (inverse iteration; NULL: not wanted; largest component positive). */
int qsim_tridiag_lowest(const double *alphas, const double *betas, int m, double *theta, double *vec);
/* Host only: what ONE step of the call above costs for these terms — the sweeps of the H application (the Pauli-sum grouping), the
 * other sweeps (2: alpha and the update) and the state volumes read and written by all of them.  QSIM_ERR_ARG for max_steps < 1. */
int qsim_lanczos_plan(const uint64_t *ham_x, long num_ham, int max_steps, int want_vector, long *sum_sweeps_per_step, long *other_sweeps_per_step,
                      double *volumes_per_step);
/* ---- reduced density matrices of qubit subsets, one read-only sweep (new) ----
 * rho[a][a'] = sum_b psi(a,b) conj(psi(a',b)); out: 4^k complex, row-major, (re, im).  Bit j of a row/column index is qubit qubits[j]
 * (qubits[0] = LSB), any order, distinct.  k = 0: the 1x1 matrix (norm^2).  k <= qsim_reduced_density_max_qubits().
 * The call settles the state first (queued gates are launched, a lazily held |0...0> or a partial support is written out), leaves
 * the state's bits alone and waits for its result.  One sweep reads the state once, whatever the subset: the 4^k sums are the
 * accumulator tiles of the fp64 matrix instruction, on a sorted subset of three to five qubits — fewer are padded with the lowest
 * index bits not in the subset and the padding is traced out on the host, which also permutes rows and columns into the caller's
 * order.  A register too small for a tile (fewer than five qubits, or fewer than four environments) takes a plain one-workgroup
 * kernel instead; qsim_reduced_density_plan says which.  The scratch of a sweep is allocated per call, before anything is launched.
 * The sums are fp64 in both precisions — fp32 amplitudes are widened on load, so a product of two floats is exact — and are added in
 * a fixed order: equal calls return equal bits.  The grid follows the rule of the other reducing sweeps and QSIM_OPT_GRID_CAP does
 * not apply (it would change the order).  The output is Hermitian bit for bit: the lower triangle is filled from the upper one and
 * the diagonal's imaginary parts are exactly 0.  Sweeps are NOT counted in the qsim_stats record (no QSIM_K_* class of their own);
 * qsim_density_sweeps_launched() counts them.  A shard that holds nothing (qsim_holds_nothing) gives zeros and launches no sweep.
 * QSIM_ERR_ARG, nothing launched: a NULL state or output, qubits NULL with k > 0, k < 0, k above the maximum or above the register's
 * qubit count, a qubit outside the register, a repeated qubit.
 * Single states only, fp64 and fp32: there is NO cluster counterpart.  Out of scope: more than five qubits (the accumulators no
 * longer fit one wave; qsim_subsystem_density below takes six to ten) and any call that writes the state (collapse). */
int qsim_reduced_density(qsim_state *s, const int *qubits, int k, double *out_re_im);
int qsim_reduced_density_max_qubits(void);   /* 5 */
/* Host only, no device: what the call above does on a register of num_q qubits held in precision_bits (64 or 32) — *path 1: the
 * matrix path, 0: the plain kernel; *padded_k and *kernel_mask: the subset the kernel works on (path 0: the caller's, nothing is
 * padded); *units_visited: the 16-byte units (one fp64 amplitude, two fp32 amplitudes) the sweep reads, the whole state once;
 * *trips_per_workgroup_at_grid_cap: the trips of a workgroup's loop when the grid is at its cap of 1024 workgroups (a device that
 * holds fewer at once makes more).  QSIM_ERR_ARG as above, and for num_q outside [0, 40], precision_bits other than 64 or 32, a NULL
 * result pointer. */
int qsim_reduced_density_plan(const int *qubits, int k, int num_q, int precision_bits, int *path, int *padded_k, uint64_t *kernel_mask,
                              uint64_t *units_visited, long *trips_per_workgroup_at_grid_cap);
uint64_t qsim_density_sweeps_launched(void); /* process-wide counter, as qsim_pauli_rotation_sweeps_launched */
/* ---- reduced density matrices of up to ten qubits: R R^T in blocks and slices on the matrix cores (new) ----
 * The same rho as qsim_reduced_density with the same conventions — bit j of a row/column index is qubit qubits[j], any order,
 * distinct; not normalised, the trace is norm^2; the call settles the state first, leaves its bits alone and waits for its result; a
 * shard that holds nothing gives zeros and launches nothing; QSIM_ERR_ARG for the same misuses — for k in [0, 10].  out: 4^k complex,
 * row-major, (re, im): 16 MiB at k = 10.  k <= 5 is forwarded to qsim_reduced_density and returns its bits (and counts there).
 * k >= 6: the real matrix R (row 2a = Re Psi[a], row 2a + 1 = Im Psi[a], a over the SORTED subset) has 2^(k+1) rows; G = R R^T is cut
 * into square blocks of 128 rows, of which only the blocks (bi <= bj) are computed, and the 2^(n-k) environments into S slices of
 * chunks of 32.  One workgroup takes one (block, slice): per chunk it stages the two row panels in LDS, widened to fp64, and its four
 * waves accumulate a 64 x 64 quarter each with the fp64 matrix instruction (of a diagonal block, symmetric itself, only the 16 x 16
 * tiles on and above its diagonal); it writes one partial block, and a final kernel adds the S partials of every element in ascending
 * slice order.  No atomics.  Block size, S and the order depend on (n, k, precision, subset)
 * alone — not on the device, QSIM_OPT_GRID_CAP or an occupancy query — so equal calls return equal bits on any device.  Products of
 * fp32 amplitudes are exact and every sum is fp64.  The state is read `blocks` = 2^(k+1) / 128 times over all workgroups (once for
 * k = 6, 16 times for k = 10); the caches take a part of that.  A register with fewer than four environments (n - k < 2) takes a plain
 * kernel, one thread per element of rho.  The host builds rho from the blocks, fills the lower triangle from the upper one, makes the
 * diagonal's imaginary parts exactly +0 and permutes rows and columns into the caller's order: Hermitian bit for bit.  Scratch (S
 * partials of every upper block and the result, at most 1 GiB) is allocated per call before anything is launched.
 * qsim_subsystem_sweeps_launched() counts the sweeps of k >= 6.  Single states only, fp64 and fp32: there is NO cluster counterpart.
 * Out of scope: more than ten qubits — beyond that the 4^k result and its diagonalisation on the host dominate the call. */
int qsim_subsystem_density(qsim_state *s, const int *qubits, int k, double *out_re_im);
int qsim_subsystem_density_max_qubits(void); /* 10 */
/* Host only, no device: what the call above does on a register of num_q qubits held in precision_bits (64 or 32) — *path 1: blocks
 * and slices, 0: the plain kernel, 2: forwarded to qsim_reduced_density (k <= 5; qsim_reduced_density_plan says what that does, the
 * fields below are 0 but for *units_read, one state volume); *block_rows: rows of R in a block (128); *upper_blocks: blocks computed;
 * *slices: S; *units_read: 16-byte units (one fp64 amplitude, two fp32 amplitudes) loaded by all workgroups together — the traffic
 * model, state volumes times the units of the state; *scratch_bytes: device scratch of the call; *trips_per_workgroup: chunks of 32
 * environments a workgroup walks (path 0: 1).  QSIM_ERR_ARG as for qsim_reduced_density_plan, with k up to 10. */
int qsim_subsystem_density_plan(const int *qubits, int k, int num_q, int precision_bits, int *path, int *block_rows, long *upper_blocks,
                                long *slices, uint64_t *units_read, uint64_t *scratch_bytes, long *trips_per_workgroup);
uint64_t qsim_subsystem_sweeps_launched(void); /* process-wide counter, as qsim_density_sweeps_launched */
/* ---- dense matrices on up to five target qubits, under controls, one in-place sweep (new) ----
 * psi <- (1 - Pi) psi + Pi (U on targets) psi, Pi = the projector on "every control qubit is 1".
 * U: 2^k x 2^k, row-major, (re, im) doubles; bit j of a row/column index is targets[j] (targets[0] = LSB, any order, as
 * qsim_reduced_density).  Any complex matrix: nothing checks unitarity (a Kraus operator, a projector).  k in [0, 5]
 * (qsim_apply_matrix_max_qubits); k == 0 is the complex scalar U[0] on the control subspace.  controls: any number of qubits, disjoint
 * from the targets; num_controls == 0 is the plain gate.  Control values of 0 are out of scope (conjugate with X).
 * The call settles the state first (queued gates are launched, a lazily held |0...0> or a partial support is written out), launches
 * ONE sweep on the state's stream that reads and writes 2^-c of the state once for c controls, and returns without waiting.  It does
 * not go through the gate queue or the fusion scheduler.  The sweep runs on the matrix cores: on a sorted subset of three to five
 * qubits (fewer targets are padded with the lowest index bits that are neither targets nor controls, U (x) 1 on the host) the real
 * matrix [[Re U, -Im U], [Im U, Re U]] meets [Re psi; Im psi] of 16 environments per fp64 matrix instruction; every lane stores the
 * rows it loaded, so there is no shared memory and no barrier, and every amplitude is written by one wave in a fixed order: equal
 * calls give equal bits whatever QSIM_OPT_GRID_CAP is.  fp32 amplitudes are widened, the sums are fp64 and each result is rounded
 * once.  A register with fewer than 16 environment units takes a plain one-workgroup kernel instead; qsim_apply_matrix_plan says
 * which.  Amplitudes outside the control subspace keep their bits.  Sweeps are NOT counted in the qsim_stats record;
 * qsim_matrix_sweeps_launched counts them.  A shard that holds nothing (qsim_holds_nothing) stays as it is and launches no sweep.
 * QSIM_ERR_ARG, nothing launched: a NULL state or U, targets NULL with k > 0, controls NULL with num_controls > 0, a negative count,
 * k above the maximum or above the register's qubit count, a qubit outside the register, a repeated qubit, a control among the
 * targets, a non-finite entry of U.
 * Single states only, fp64 and fp32: there is NO cluster counterpart (sharded states have no controlled operations).  Out of scope:
 * more than five targets, gradients through these gates. */
int qsim_apply_matrix(qsim_state *s, const double *U, const int *targets, int k, const int *controls, int num_controls);
int qsim_apply_matrix_max_qubits(void);      /* 5 */
/* Host only, no device: what the call above does on a register of num_q qubits held in precision_bits (64 or 32) — *path 1: the
 * matrix path, 0: the plain kernel; *padded_k and *kernel_mask: the sorted subset the kernel works on (path 0: the targets, nothing
 * is padded); *units: the 16-byte units (one fp64 amplitude, two fp32 amplitudes) the sweep reads and writes, 2^-c of the state
 * (fp32 with a control on qubit 0: the odd amplitude of 2^(1-c) of the units); *trips_per_workgroup: the trips of a workgroup's loop
 * at the default grid's cap (1024 workgroups, 512 for five qubits; a device that holds fewer at once makes more).  QSIM_ERR_ARG as
 * above, and for num_q outside [0, 40], precision_bits other than 64 or 32, a NULL result pointer. */
int qsim_apply_matrix_plan(const int *targets, int k, const int *controls, int num_controls, int num_q, int precision_bits, int *path,
                           int *padded_k, uint64_t *kernel_mask, uint64_t *units, long *trips_per_workgroup);
/* Host only: the real operand M the matrix path's kernel is handed for this call (*rows x *rows, row-major, *rows = 2^(padded_k + 1),
 * at most 64) and which row of [Re psi; Im psi] each of its rows and columns is: row_amp[r] an index over the sorted kernel_mask,
 * row_part[r] 0 Re, 1 Im.  Lane l of a wave supplies and receives the rows r with r mod 4 == l / 16.  The plain path has no operand:
 * *rows = 0.  QSIM_ERR_ARG as above. */
int qsim_apply_matrix_operand(const double *U, const int *targets, int k, const int *controls, int num_controls, int num_q,
                              int precision_bits, double *M, int *row_amp, int *row_part, int *rows);
uint64_t qsim_matrix_sweeps_launched(void);  /* process-wide counter, as qsim_density_sweeps_launched */
/* ---- permutations of the basis states of up to ten target qubits, under controls, one in-place sweep (new) ----
 * A classical reversible function on a register: for every environment e (the index bits outside the targets) in which every control
 * qubit is 1,  new[e | dep(perm[j])] = old[e | dep(j)],  dep putting bit i of its argument on qubit targets[i].  It is qsim_apply_matrix
 * with U[perm[j]][j] = 1 without the arithmetic: amplitudes are moved bit for bit, in fp64 and in fp32, and nothing is rounded.
 * perm: 2^k entries, a bijection of [0, 2^k); bit i of an entry and of its position is targets[i] (targets[0] = LSB, any order).  k in
 * [0, 10] (qsim_apply_permutation_max_qubits); k == 0 takes the table {0}.  controls: any number of qubits, disjoint from the targets.
 * The call settles the state first (queued gates are launched, a lazily held |0...0> is written out), sends the operand through a
 * pinned ring to the state's sweep scratch, launches ONE sweep on the state's stream that reads and writes 2^-c of the state once, and
 * returns without waiting.  It does not go through the gate queue or the fusion scheduler.  The identity table is swept like any other.
 * The sweep works tile by tile: a tile is B index bits — the targets and the lowest index bits that are neither targets nor controls,
 * B = min(12, n - c) for fp64 and min(13, n - c) for fp32, 64 KiB of amplitudes at most.  A workgroup loads a tile with coalesced loads,
 * writes each amplitude into shared memory at its destination, and stores the tile back linearly to the addresses it loaded; a tile
 * holds every target, so it is closed under the map and the sweep needs no second buffer.  Each amplitude is written by one thread:
 * equal calls give equal bits whatever QSIM_OPT_GRID_CAP is.  Amplitudes outside the control subspace are neither read nor written.
 * Sweeps are NOT counted in the qsim_stats record; qsim_permutation_sweeps_launched counts them, one per accepted call.  A shard that
 * holds nothing (qsim_holds_nothing) stays as it is and launches no sweep.
 * QSIM_ERR_ARG, nothing launched and the state untouched: a NULL state or table, targets NULL with k > 0, controls NULL with
 * num_controls > 0, a negative count, k above the maximum or above the register's qubit count, a qubit outside the register, a repeated
 * qubit, a control among the targets, an entry of the table >= 2^k, two equal entries.
 * Single states only, fp64 and fp32: there is NO cluster counterpart.  Out of scope: phases on the moved amplitudes (a monomial
 * matrix; its table would follow the map in the scratch), gradients through these calls. */
int qsim_apply_permutation(qsim_state *s, const uint32_t *perm, const int *targets, int k, const int *controls, int num_controls);
int qsim_apply_permutation_max_qubits(void); /* 10 */
/* Host only, no device: what the call above does on a register of num_q qubits held in precision_bits (64 or 32) — *path 1: whole
 * tiles of 12 (fp64) or 13 (fp32) bits; 0: n - c is smaller, the one tile is the whole control subspace and one workgroup runs the
 * same kernel with runtime bounds; *tile_bits: B; *tile_mask: the tile's index bits; *tiles: 2^(n - c - B); *units: the 16-byte units
 * read and written once (fp64: 2^(n - c); fp32: half as many, an amplitude being 8 bytes; never below 1); *trips_per_workgroup: the
 * tiles a workgroup walks at the default grid's cap of 512 workgroups (a device that holds fewer at once makes more).  QSIM_ERR_ARG as
 * above, and for num_q outside [0, 40], precision_bits other than 64 or 32, a NULL result pointer. */
int qsim_apply_permutation_plan(const int *targets, int k, const int *controls, int num_controls, int num_q, int precision_bits, int *path,
                                int *tile_bits, uint64_t *tile_mask, uint64_t *tiles, uint64_t *units, long *trips_per_workgroup);
/* Host only: exactly the array the device is handed for this call — local_map[u] for every tile-local index u in [0, *entries),
 * *entries = 2^B (room for 8192 is enough): bit i of u is the i-th lowest bit of tile_mask; the target bits of u go through perm (the
 * caller's order against the sorted one), the padding bits are kept.  QSIM_ERR_ARG as above. */
int qsim_apply_permutation_operand(const uint32_t *perm, const int *targets, int k, const int *controls, int num_controls, int num_q,
                                   int precision_bits, uint16_t *local_map, int *entries);
uint64_t qsim_permutation_sweeps_launched(void); /* process-wide counter, as qsim_density_sweeps_launched */
/* ---- whole-register diagonal operators from a table: exp(-i gamma D) and <D>, <D^2> in one sweep each (new) ----
 * A qsim_diagonal is a real table d[0..2^n) of fp64 on one device, the operator D = sum_i d_i |i><i| on a register of n qubits: a
 * cost function of QAOA, a penalty, a marked set, a potential on a grid — whatever the number of Pauli terms it would take.  The
 * table is fp64 for fp64 and fp32 states alike.  Single states only: there is NO cluster counterpart.
 * Ordering: calls take effect in the order issued, as if on one stream, and the caller synchronises nothing.  The calls that fill or
 * inspect a table (add_terms, write, read, extrema) wait for every sweep that still reads it, run on a stream of the table's own and
 * have finished when they return (they block the host); the two sweeps run on the state's stream and never wait on the host.
 * Out of scope: controls on the phase, gradients with respect to gamma, sharded tables, complex tables. */
typedef struct qsim_diagonal qsim_diagonal;
/* 2^num_q doubles, all 0, for num_q in [0, 40]; QSIM_ERR_ALLOC when the allocation fails, QSIM_ERR_ARG for num_q or device out of range */
int qsim_diagonal_create(qsim_diagonal **out, int num_q, int device);
/* The same on the caller's buffer of 2^num_q doubles on `device` (aligned to 16 bytes), as qsim_create_external adopts a state's: how
 * a table computed on the device gets in.  Nothing is zeroed and nothing is ever freed; the caller keeps the buffer alive while the
 * object lives and orders its own work on the buffer against these calls (its writes finished before a call, none during a sweep). */
int qsim_diagonal_create_external(qsim_diagonal **out, int num_q, int device, void *device_doubles);
void qsim_diagonal_destroy(qsim_diagonal *d);              /* waits for the sweeps that read the table; NULL is allowed */
int qsim_diagonal_num_qubits(const qsim_diagonal *d);      /* -1 for NULL */
void *qsim_diagonal_device_ptr(qsim_diagonal *d);          /* the 2^n doubles in HBM; NULL for NULL */
/* d_i <- (...((d_i + c_0 s_0(i)) + c_1 s_1(i)) + ...) with s_k(i) = (-1)^popcount(i & z_masks[k]): the diagonal of sum_k c_k P_k for
 * strings P_k of I and Z, added term after term in the caller's order.  c s is an exact sign flip, so the table is bit for bit the
 * sequential sum, whatever the grid.  z == 0 adds a constant.  The terms travel to the kernel by value in records of at most 32, one
 * launch — one read and one write of the table — per record; nothing is allocated.  num_terms == 0 does nothing.
 * QSIM_ERR_ARG, the table unchanged: a NULL table, NULL arrays with num_terms > 0, a negative count, a mask bit at or above n. */
int qsim_diagonal_add_terms(qsim_diagonal *d, const uint64_t *z_masks, const double *coeffs, long num_terms);
/* entries [first, first + count) from and to host memory; QSIM_ERR_ARG for a range outside the table or a NULL pointer with count > 0 */
int qsim_diagonal_write(qsim_diagonal *d, uint64_t first, uint64_t count, const double *host);
int qsim_diagonal_read(qsim_diagonal *d, uint64_t first, uint64_t count, double *host);
/* The smallest and the largest entry and where they are, one read-only reduction: the optimum of a cost function, the scale of an
 * approximation ratio.  Among equal values the LOWEST index is returned, and equal calls return equal results.  A table that holds a
 * NaN gives unspecified results. */
int qsim_diagonal_extrema(qsim_diagonal *d, double *min, uint64_t *argmin, double *max, uint64_t *argmax);
/* a_i <- exp(-i gamma d_i) a_i for every amplitude, in place, in ONE sweep that reads the state and the table and writes the state.
 * With D = sum_k c_k P_k built by qsim_diagonal_add_terms the call equals qsim_apply_pauli_rotations with theta_k = 2 gamma c_k.
 * The factor is formed in fp64 for both precisions, by sincospi of (gamma / pi) d_i — exact argument reduction, whatever the
 * magnitude — rounded once to the state's precision and multiplied in that precision.  The call settles the state first (queued gates
 * are launched, a lazily held |0...0> or a partial support is written out: afterwards the state is dense), launches on the state's
 * stream and returns without waiting; it allocates nothing and every amplitude is written by one thread: equal calls give equal bits.
 * Sweeps are NOT counted in the qsim_stats record; qsim_diagonal_sweeps_launched counts them.  A shard that holds nothing
 * (qsim_holds_nothing) stays as it is and launches no sweep.
 * QSIM_ERR_ARG, nothing launched: a NULL argument, a table over another number of qubits or on another device, a non-finite gamma. */
int qsim_apply_diagonal_phase(qsim_state *s, const qsim_diagonal *d, double gamma);
/* out[0] = sum_i d_i |a_i|^2 = <D> and out[1] = sum_i d_i^2 |a_i|^2 = <D^2> (for the variance), one read-only sweep after the queued
 * gates; the state's bits stay as they are.  The sums are fp64 in both precisions and are added in a fixed order: equal calls return
 * equal bits.  A shard that holds nothing gives zeros and launches no sweep.  QSIM_ERR_ARG as above, and for a NULL out. */
int qsim_expect_diagonal(qsim_state *s, const qsim_diagonal *d, double out[2]);
uint64_t qsim_diagonal_sweeps_launched(void); /* process-wide counter of the two sweeps above (not of the calls that fill a table) */
/* Host only, no device: how the two sweeps walk a register of num_q qubits held in precision_bits (64 or 32).  *items: the work
 * items, one 16-byte unit of the table = two amplitudes each (1 for a register of one amplitude); *items_per_trip_*: items per thread
 * and trip of a workgroup's loop; *trips_at_cap_*: the trips of that loop when the grid is at its cap (2048 workgroups for the phase
 * sweep, 1024 for the expectation sweep; a device that holds fewer at once makes more).  Registers of fewer than 128 amplitudes take
 * a plain path of one workgroup and one trip.  QSIM_ERR_ARG for num_q outside [0, 40], precision_bits other than 64 or 32, a NULL
 * result pointer. */
int qsim_diagonal_plan(int num_q, int precision_bits, uint64_t *items, int *items_per_trip_phase, int *items_per_trip_expect,
                       long *trips_at_cap_phase, long *trips_at_cap_expect);
/* ---- adjoint-mode gradients through diagonal phases, and <D> as (part of) the observable (new) ----
 * qsim_controlled_pauli_gradient for a circuit whose steps are Pauli rotations OR diagonal phases: step k with step_diag[k] != NULL is
 * exp(-i angles[k] D_k) for that table (qsim_apply_diagonal_phase), and grad[k] = dE/dgamma_k = 2 sum_i d_i Im(conj(lambda_i) psi_i);
 * every other step is the (controlled) rotation of step_c, step_x, step_z and angles[k] = theta_k.  step_c, step_x and step_z of a
 * diagonal step are not looked at, except that a non-zero control mask there is refused.  step_diag NULL: no diagonal step.
 * H = sum_t coeffs[t] Q_t + obs_weight D_obs; obs NULL: no diagonal part (obs_weight is not looked at); num_ham may be 0.
 * One forward pass (a diagonal step is one sweep, rotations between two diagonal steps fuse as in qsim_apply_pauli_rotations), lambda =
 * H psi (the Pauli sweeps, then one sweep for the diagonal part), the energy, and the backward pass: one sweep per diagonal step, which
 * reads psi, lambda and the table, and the sweeps of qsim_pauli_gradient for each run of rotations between them.  The state is left as
 * the call found it, to rounding; a list of diagonal steps only leaves the bits that qsim_apply_diagonal_phase with gamma_1 .. gamma_K
 * and then -gamma_K .. -gamma_1 leaves.  Equal calls return equal bits.  A shard that holds nothing: energy 0, gradient zeros, no sweep.
 * A call without diagonal steps and without obs launches exactly what qsim_controlled_pauli_gradient launches.
 * QSIM_ERR_ARG, the state untouched: what qsim_controlled_pauli_gradient refuses; a table of another qubit count or on another device;
 * a non-finite angle or obs_weight; a control mask on a diagonal step; NULL arguments or negative counts.
 * Backward diagonal sweeps count in qsim_diagonal_adjoint_sweeps_launched only; forward phases and the D_obs sweep in
 * qsim_diagonal_sweeps_launched; the rotations' backward sweeps in qsim_pauli_adjoint_sweeps_launched. */
int qsim_diagonal_gradient(qsim_state *s, long num_steps,
        const qsim_diagonal *const *step_diag, /* [num_steps], NULL entry = Pauli rotation; NULL array = none */
        const uint64_t *step_c,                /* NULL = no controls anywhere */
        const uint64_t *step_x, const uint64_t *step_z, const double *angles, /* theta_k or gamma_k */
        const uint64_t *ham_x, const uint64_t *ham_z, const double *coeffs, long num_ham,
        const qsim_diagonal *obs, double obs_weight, /* obs NULL = no diagonal part */
        double *energy, double *grad /* [num_steps] */);
/* Host only, no device: the sweeps qsim_diagonal_gradient makes after its forward pass.  is_diag[k] != 0: step k is a diagonal phase
 * (NULL: none is).  *pauli_adjoint_sweeps: the rotations' backward sweeps — a run never fuses across a diagonal step;
 * *diag_adjoint_sweeps: one per diagonal step; *sum_sweeps: the Pauli sweeps of lambda = H psi plus one for the diagonal part (has_obs);
 * *diag_adjoint_items_per_trip and *diag_adjoint_trips_at_cap: as qsim_diagonal_plan reports them, for the backward diagonal sweep (its
 * grid holds 1024 workgroups at most).  QSIM_ERR_ARG as for qsim_controlled_gradient_plan, and for a control mask on a diagonal step. */
int qsim_diagonal_gradient_plan(const unsigned char *is_diag, const uint64_t *step_c, const uint64_t *step_x, long num_steps,
        const uint64_t *ham_x, long num_ham, int has_obs, int num_q, int precision_bits,
        long *pauli_adjoint_sweeps, long *diag_adjoint_sweeps, long *sum_sweeps,
        int *diag_adjoint_items_per_trip, long *diag_adjoint_trips_at_cap);
uint64_t qsim_diagonal_adjoint_sweeps_launched(void); /* process-wide counter of the backward diagonal sweeps */
/* dst (device, 2^n amplitudes of the state's precision, not the state's own buffers) = weight D |state>, or += with accumulate != 0:
 * one out-of-place sweep on qsim_stream(), not waited for; weight d_i is rounded once to the state's precision.  When storing, dst's
 * old contents are not read.  Counts in qsim_diagonal_sweeps_launched.  QSIM_ERR_ARG as for qsim_apply_diagonal_phase (weight in
 * gamma's place), and for dst_device NULL or equal to the state's buffer or its spare buffer. */
int qsim_diagonal_apply_into(qsim_state *s, const qsim_diagonal *d, double weight, void *dst_device, int accumulate);
void *qsim_device_ptr(qsim_state *s);        /* amplitude array in HBM: launches pending gates and writes a lazily held
                                              * |0...0> first (work is queued on qsim_stream(), not waited for); NULL on error */
void *qsim_stream(qsim_state *s);            /* the hipStream_t every launch goes to */

/* ---- measurement post-path (dead code in the reference's main, quantum_simulator.c:67-73) ---- */
/* compute_state_cumulative_distribution + the search of measurement (quantum_simulator.c:256-283) without ever
 * materialising the 2^n-entry cumulative array: |a|^2 is summed per block of 4096 amplitudes on the device, the
 * block sums are prefix-summed on the host, and only the block a draw falls into is scanned.  For every random
 * number in randoms[0..shots) the result is the first basis index whose cumulative probability is non-zero and
 * not below it, or 2^n - 1 (exactly the reference's loop; summation order differs from its strictly sequential
 * one, so a draw within ~1e-15 of a boundary may land on the neighbouring index). */
int qsim_sample(qsim_state *s, const double *randoms, long shots, uint64_t *out_indices);
/* The random number measurement() draws (:271-276): ten rand() values, each scaled by a further 1/RAND_MAX. */
double qsim_draw_randn(void);
/* putb (:285-293): `len` binary digits of n, most significant first, NUL-terminated into buf (len + 1 bytes). */
void qsim_putb(long long n, int len, char *buf);

/* ---- shots drawn on the device (one state only — a cluster keeps qsim_cluster_sample) ----
 * qsim_sample above restates the reference for a handful of draws: a blocking copy and a host scan per draw.  qsim_sample_shots draws
 * any number of shots in one read-only sweep of the state plus one wave per draw, and never writes the cumulative distribution at
 * amplitude resolution.  It keeps a pyramid of fp64 sums instead (both precisions; p_i = fma(re, re, im im) on widened components):
 * chunks of 2^cb amplitudes, cb = min(8, n), which one wave scans in a fixed order; groups of 2^gb amplitudes, gb = min(18, n), with
 * the running sums of their chunks' totals; and the running sums of the groups' totals.  Both running sums are sequential, so they
 * never decrease.  A draw u in [0, 1] becomes r = u T, T the state's own total; the first group and then the first chunk whose running
 * sum is non-zero and >= r are found by bisection, the chunk is scanned again by the same code that formed its total, and the result is
 * the chunk's first index i with p_i > 0 whose cumulative value is non-zero and >= r.  The chunk's end and the bisected sums round
 * differently, so rounding can leave no such index: then the result is the chunk's LAST index with p_i > 0 (there is one: the chunk
 * moved the running sum).  What follows, and where it departs from qsim_sample:
 *   - draws are scaled by the state's total, so an unnormalised state samples |a_i|^2 / sum |a|^2 (qsim_sample compares the random
 *     number with the unscaled cumulative sum and piles what lies beyond it on 2^n - 1);
 *   - an index of probability zero is never returned, and there is no fallback index: u = 0 returns the first index with p > 0, u = 1
 *     an index of the last chunk that moved the total, never a blind 2^n - 1;
 *   - a draw within rounding of a boundary of the cumulative distribution (about 2^(n-52) T) may land on either side of it, as for
 *     qsim_sample, whose order of summation is another one;
 *   - every result depends only on the state's bits and the draw: equal calls return equal bits whatever QSIM_OPT_GRID_CAP is (it caps
 *     all three kernels), and the state's bits are untouched.  No atomics.
 * The scratch — 8 bytes per chunk and per group, 0.2 % of an fp64 state — and 16 bytes per draw are allocated and freed by the call. */
/* Host only, no device: the pyramid of a register of n qubits (0 to 40): *chunk_bits = min(8, n), *group_bits = min(18, n),
 * *scratch_bytes = 8 (2^(n - cb) + 2^(n - gb)).  QSIM_ERR_ARG for n outside 0..40 or a NULL pointer. */
int qsim_sample_geometry(int n, int *chunk_bits, int *group_bits, uint64_t *scratch_bytes);
/* out[k] for draws[k] in [0, 1], k < shots: the basis index, or with num_qubits > 0 the outcome on `qubits` — bit j of out[k] is bit
 * qubits[j] of the index.  Launches pending gates first (deferred X flips included), uploads the draws, runs the three kernels on
 * qsim_stream(), copies the results back and waits.  shots == 0 is QSIM_OK and launches nothing.  QSIM_ERR_ARG, before any launch: a
 * NULL pointer (qubits may be NULL with num_qubits == 0), shots < 0, a draw outside [0, 1] or NaN, more than 64 qubits, a qubit outside
 * the register or listed twice.  QSIM_ERR_ARG also for a state whose total is 0 (or not finite): nothing is written to out then. */
int qsim_sample_shots(qsim_state *s, const double *draws, long shots, const int *qubits, int num_qubits, uint64_t *out);
/* For measurements (tools/sample_bench.py): runs the two preparing stages of qsim_sample_shots once on a pyramid of its own and reports
 * what device events around them say, in milliseconds: the chunk-sum sweep, and the two launches of the prefix kernel.  Waits. */
int qsim_sample_stage_times(qsim_state *s, double *chunk_sums_ms, double *prefix_ms);

/* ---- measured pass geometry (planning, in the sense of FFTW's wisdom) -------------------------------------------------
 * A cache-blocked pass walks nine "high" index bits besides the contiguous low ones; which of them the lanes of a wave,
 * the waves of a workgroup and the registers of a lane walk changes nothing in the result and up to 2x in the pass's
 * HBM time.  qsim_tune_circuit plans `circuit` as qsim_run_circuit would and times every pass of
 * the schedule under up to max_candidates orders of its bits (ascending first, then seeded permutations; budget_ms
 * bounds the total, 0 = unbounded); the fastest order per (register size, precision, tile shape, bit set) is kept in
 * a process-wide table that every later run with that geometry uses.  The state's contents are clobbered: it is left
 * reset to |0...0>.  Not part of any timed region — call it once per circuit shape, like building a plan. */
typedef struct {
    int tile_passes;      /* tile passes in the circuit's schedule */
    int already_known;    /* ... whose geometry was in the table already */
    int passes_tuned;     /* ... measured now */
    int passes_reordered; /* ... for which an order beat ascending by more than the timing noise */
    int candidates_timed;
    double ms_ascending;  /* sum over the measured passes: time in ascending order */
    double ms_best;       /* ... and in the order kept */
    double seconds;       /* wall time spent measuring */
} qsim_tune_report;
int qsim_tune_circuit(qsim_state *s, const qsim_circuit *circuit, int max_candidates, double budget_ms, qsim_tune_report *report);
/* Only the first half of that planning step, without any timing: schedules the circuit under a handful of scheduler
 * settings (clusters that commute may or may not overtake each other, ...), keeps the one whose passes move the fewest
 * bytes for this circuit — for a run from a reset and for a run on a dense state — and returns.  qsim_tune_circuit does
 * this too. */
int qsim_choose_schedule(qsim_state *s, const qsim_circuit *circuit);
/* The same choice for a run from a reset, for as long as the buffer of a state made by qsim_create_async is still being allocated
 * and no longer: the candidates scheduled by then compete (on up to 16 host threads), the default always does.  Returns at
 * once when the buffer is there already.  What bin/qsim does between the parse and the first launch. */
int qsim_choose_schedule_while_allocating(qsim_state *s, const qsim_circuit *circuit);
/* The same for a circuit that will run on a state that is NOT fresh from a reset (dense_start != 0): the schedule of such a
 * run differs in its first passes (QSIM_OPT_SPARSE_START), e.g. a shard's local gates after its first exchange. */
int qsim_tune_circuit_from(qsim_state *s, const qsim_circuit *circuit, int max_candidates, double budget_ms, qsim_tune_report *report,
                           int dense_start);
/* Both for a run that finds the state with exactly the support `support` (index bits that may be 1: 0 fresh from a reset, all
 * ones dense, the mask given to qsim_set_support after a sparse exchange): a shard's local steps between exchanges. */
int qsim_choose_schedule_for(qsim_state *s, const qsim_circuit *circuit, uint64_t support);
/* Index bits that may be 1 somewhere in the state after `circuit` ran on a state with support `support`, as the engine itself
 * will track it (the circuit is scheduled as qsim_flush will schedule it, remembered schedule choice included; nothing runs). */
int qsim_support_after(qsim_state *s, const qsim_circuit *circuit, uint64_t support, uint64_t *after);
int qsim_tune_circuit_support(qsim_state *s, const qsim_circuit *circuit, int max_candidates, double budget_ms, qsim_tune_report *report, uint64_t support);
long qsim_tune_table_size(void);
void qsim_tune_table_clear(void);
int qsim_tune_table_save(const char *path);  /* text, one geometry per line */
long qsim_tune_table_load(const char *path); /* entries loaded (malformed lines are skipped), -1 if the file cannot be read */

/* ---- sharded states (new: the reference is single-device) --------------------------------
 * A qsim_state may hold one contiguous shard of a larger register: the caller (one process per GPU)
 * keeps the top log2(P) index bits as the rank id and owns the logical->physical qubit map.
 * qsim_pack_bits re-lays the shard out ahead of a global<->local qubit exchange:
 *     dst[(block << (n-k)) | rest] = amps[src],  block = the k bits of src at positions bits[0..k)
 *                                                (ascending), rest = the other n-k bits in order,
 * so block b is the contiguous piece rank-group member b must receive (RCCL send/recv or all-to-all of
 * 16<<(n-k) byte blocks over xGMI).  dst is caller-owned device memory of 16<<n bytes. */
int qsim_pack_bits(qsim_state *s, const int *bits, int nbits, void *dst_device);
/* The same re-layout with one destination per block (nbits <= 3): block b is written to dst_blocks[b] (2^(n-k)
 * amplitudes each), e.g. straight into the spare buffer of the group member that will own it — another shard's buffer
 * on the same device or a peer-mapped one — so that pack and transfer are one kernel.  qsim_swap_buffer then makes the
 * spare buffer (now holding the shard's new contents) the state and hands back the old one. */
int qsim_pack_bits_to(qsim_state *s, const int *bits, int nbits, void *const *dst_blocks);
int qsim_swap_buffer(qsim_state *s, void **buffer_device);
/* The receiving side of an exchange knows where its new contents can be non-zero (a run starts from |0...0>, and a qubit
 * stays |0> until a gate mixes it): qsim_set_support declares every amplitude whose index has a bit outside `support` zero BY
 * DEFINITION — that memory need not have been written — which is the state the first tile passes of a run leave behind
 * (QSIM_OPT_SPARSE_START): later tile passes visit only that part, anything else gets the zeros written out first.
 * qsim_get_support reports the current situation without touching the buffer: *support = index bits that may be 1 (all
 * ones: dense), *kind = 1 while the state is a basis state amp0 * |0...0> that no kernel has written yet (amp0 = 0: the
 * all-zero vector of a shard that holds nothing — gates applied to it are dropped), else 0.
 * qsim_pack_bits_sparse is qsim_pack_bits / qsim_pack_bits_to (dst_blocks != NULL) without the detour of writing the zeros out
 * first: amplitudes outside the state's support are packed as zeros straight away (never loaded), and the blocks in skip_blocks
 * (bit b: block b; its destination may be NULL) are not written at all — nobody will look at them.
 * qsim_state_buffer: the amplitude buffer as is — nothing launched, nothing written (for a caller about to overwrite it). */
int qsim_set_support(qsim_state *s, uint64_t support);
int qsim_get_support(qsim_state *s, uint64_t *support, int *kind, double *amp0);
/* 1 when the state is the all-zero vector of a shard that holds nothing (qsim_reset_shard(s, 0), nothing written since); does
 * not flush. */
int qsim_holds_nothing(const qsim_state *s);
int qsim_pack_bits_sparse(qsim_state *s, const int *bits, int nbits, void *dst_device, void *const *dst_blocks, uint32_t skip_blocks);
void *qsim_state_buffer(qsim_state *s);
/* qsim_flush and the re-layout of qsim_pack_bits_sparse in ONE call: when the last pass of the queue is a tile pass of the
 * default shape, its stores write the state re-laid-out (*fused = 1) and the exchange costs no sweep of its own; otherwise the
 * passes run as usual and the pack kernel follows (*fused = 0).  The output is one buffer (`out`; NULL: the state's spare
 * buffer) in which source index bit bits[j] lands on bit to_bits[j] (NULL: num_q - nbits + j, i.e. the block index on top of
 * a shard-sized buffer), the other bits close ranks below, and konst is ORed into the index (a cluster that keeps every
 * shard's buffer in one allocation addresses "block b of member j" that way).  needed: source index bits that may be 1 where
 * the receivers expect data (a fusing pass over a partially written state only writes inside its support; if that does not
 * cover `needed` the pack kernel, which writes the zeros, is used).  nbits = 4..8 (groups of 16 and more shards) and fp32
 * states always take the pack kernel (*fused = 0) and only know the one-buffer layout (to_bits NULL, konst 0).  Afterwards the state's own buffer holds stale data:
 * hand it its new contents (receives, qsim_swap_buffer) and say what they are (qsim_set_support / qsim_reset_shard). */
int qsim_flush_pack(qsim_state *s, const int *bits, int nbits, const int *to_bits, uint64_t konst, void *out_device, uint64_t needed,
                    uint32_t skip_blocks, void **packed_at, int *fused);
/* Lends the state a second device buffer of 2^n amplitudes for out-of-place tile passes (QSIM_OPT_PINGPONG) — e.g. the
 * exchange scratch of a sharded run, idle between exchanges.  The caller keeps ownership; between qsim_flush / qsim_sync
 * and the next gate the buffer is the caller's to use (its contents are garbage).  NULL takes it back. */
int qsim_set_spare_buffer(qsim_state *s, void *buffer_device);
/* Block sums / block contents for blocks that are bit-deposits instead of ranges: block w = the amplitudes at
 * deposit(w, hi_mask) | deposit(i, lo_mask), i = 0 .. 2^popcount(lo_mask) - 1 (deposit spreads the low bits of its first
 * argument over the set bits of the mask, lowest first; the masks are disjoint).  After exchanges a LOGICAL block of the
 * measurement post-path (quantum_simulator.c:256-283) is such a set of a shard's local positions: the sums are formed
 * on the device and only 2^popcount(hi_mask) doubles, or one block, reach the host.
 *   qsim_block_prob_masked: out[w] = sum_i |a|^2             qsim_gather_masked: out[i] = a[base | deposit(i, lo_mask)] */
int qsim_block_prob_masked(qsim_state *s, uint64_t hi_mask, uint64_t lo_mask, double *out_host);
int qsim_gather_masked(qsim_state *s, uint64_t base, uint64_t lo_mask, double *out_host_re_im);
/* Multiplies every amplitude of the shard by (re, im): a diagonal gate on a global qubit is a per-rank scalar. */
int qsim_scale(qsim_state *s, double re, double im);

/* ---- clusters: P = 2^p shards driven by ONE process (the C host's multi-GPU path) --------------------------
 * Each shard is a qsim_state on devices[r] (NULL: round-robin over the visible devices; the same device may
 * repeat, which gives "virtual shards" for validation on fewer GPUs).  qsim_cluster_run_circuit plans the
 * circuit (logical->physical qubit map, communication-free handling of diagonal gates / controls on global
 * qubits, Belady choice of the qubits that become global) and executes it: local steps through the ordinary
 * engine, exchanges as qsim_pack_bits + device-to-device block copies.  The one-process-per-GPU driver
 * (gpu_quantum_simulator_amd/distributed.py) runs the same plan with RCCL send/recv. */
typedef struct qsim_cluster qsim_cluster;
int qsim_cluster_create(qsim_cluster **out, int num_q, int num_shards, const int *devices);
void qsim_cluster_destroy(qsim_cluster *c);
int qsim_cluster_num_shards(const qsim_cluster *c);
qsim_state *qsim_cluster_shard(qsim_cluster *c, int shard);
int qsim_cluster_set_option(qsim_cluster *c, int option, long value);
int qsim_cluster_reset(qsim_cluster *c); /* |0...0>, identity qubit map */
/* ONE circuit per reset (compute_state_vector semantics): the plan's free first qubit placement and its sparse exchanges are
 * only right from |0...0>, so a call that does not follow qsim_cluster_reset fails with QSIM_ERR_ARG instead of dropping data.
 * What is checked is that no circuit has run since the reset: amplitudes written into a shard through qsim_cluster_shard() after
 * the reset are not noticed, and the run may drop them. */
int qsim_cluster_run_circuit(qsim_cluster *c, const qsim_circuit *circuit);
int qsim_cluster_sync(qsim_cluster *c);
/* Planning for a circuit the cluster will run (repeatedly): the shard plan is built and kept, and every shard's local steps go
 * through the schedule choice of qsim_choose_schedule — and, with max_candidates > 1, through the measured tile-bit orders of
 * qsim_tune_circuit (budget_ms for all shards together, 0 = unbounded) — each for the support the shard will have at that
 * point of the run.  The steps are planned in order for all shards, and every exchange of the kept plan is told what its
 * senders will have written under the schedules chosen (qsim_support_after), so that their last tile pass can do the
 * re-layout.  Outside any timed region; results never depend on it.  Leaves the cluster reset.
 * QSIM_TRACE_PACK=1 in the environment: one line on stderr for every re-layout that needed a sweep of its own, with the reason. */
int qsim_cluster_plan(qsim_cluster *c, const qsim_circuit *circuit, int max_candidates, double budget_ms);
int qsim_cluster_read(qsim_cluster *c, uint64_t logical_first, uint64_t count, double *out_re_im);
int qsim_cluster_norm2(qsim_cluster *c, double *out);
/* qsim_expect_paulis on a sharded state; masks are in LOGICAL qubits and are mapped through the cluster's qubit map.  Z on a
 * qubit that is a shard-id bit is a sign per shard; X or Y there pairs shard r with shard r ^ x_rank, whose buffer is read in
 * place.  That needs every shard on ONE device (virtual shards): with shards on different devices such a term is refused with
 * QSIM_ERR_ARG — a path that reads a peer's buffer or copies it over is missing — and terms whose X and Y sit on local qubits
 * work on any placement.  Every shard is flushed and its stream waited for first; per-shard results are added in shard order. */
int qsim_cluster_expect_paulis(qsim_cluster *c, const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, double *out);
/* qsim_apply_pauli_rotations on a sharded state (fp64, as clusters are); masks are in LOGICAL qubits and are mapped through the
 * cluster's qubit map.  Z on a qubit that is a shard-id bit is a sign per shard (it flips the sign of sin(theta/2) there).  X or Y
 * there pairs shard r with shard r ^ x_rank: the member with the lower id sweeps all its local indices against the partner's buffer
 * and writes both.  That needs every shard on ONE device (virtual shards): with shards on different devices such a term is refused
 * with QSIM_ERR_ARG, the restriction of qsim_cluster_expect_paulis, and terms whose X and Y sit on local qubits work on any
 * placement.  Before a cross-shard sweep every shard is flushed and its stream waited for; afterwards the partner's stream waits
 * for the sweep.  A single X or Y on a LOCAL qubit is queued on every shard as its 2x2.  The cluster no longer counts as holding
 * |0...0>: qsim_cluster_run_circuit needs a qsim_cluster_reset first. */
int qsim_cluster_apply_pauli_rotations(qsim_cluster *c, const uint64_t *x_masks, const uint64_t *z_masks, const double *thetas, long num_terms);
/* qsim_sample for a sharded state: basis indices in LOGICAL order for random numbers in [0,1] (measurement(),
 * quantum_simulator.c:270-283), whatever qubit map the exchanges left behind.  Every shard forms the |a|^2 sums of the
 * logical 2^12-amplitude blocks it holds a part of on its own device (qsim_block_prob_masked); the host adds the P
 * partial sums per block in shard order and fetches only the blocks the draws land in (qsim_gather_masked). */
int qsim_cluster_sample(qsim_cluster *c, const double *randoms, long shots, uint64_t *out_indices);
int qsim_cluster_exchange_stats(const qsim_cluster *c, uint64_t *exchanges, double *bytes_per_shard); /* bytes: if every block travelled */
/* What all shards together really sent: blocks of shards that hold nothing yet, and blocks for shards that will hold nothing
 * afterwards, stay home (a run starts from |0...0>; qsim_shard_plan_step_support). */
int qsim_cluster_exchange_bytes_moved(const qsim_cluster *c, double *bytes_all_shards);
/* Re-layouts so far, per shard and exchange: done by the last tile pass in front of the exchange / by the pack kernel. */
int qsim_cluster_pack_counts(const qsim_cluster *c, uint64_t *fused, uint64_t *separate);
/* How this cluster moves blocks: "rccl" (every shard on its own device: one ncclGroup of ncclSend/ncclRecv per exchange,
 * stream-ordered), "direct" (all shards on one device: the pack kernel writes into the members' buffers, which then
 * change roles), "copies" (mixed placements: pack + device-to-device copies) or "none" (one shard). */
const char *qsim_cluster_exchange_mode(const qsim_cluster *c);
const char *qsim_cluster_error(void);
/* The plan as an object (host only).  This is what the one-process-per-GPU driver executes: every rank builds the same
 * plan, applies its own local steps with qsim_shard_plan_apply_local on its shard state and performs the exchanges
 * (qsim_pack_bits + send/recv of the blocks) itself.  step kinds: 0 local, 1 exchange (k shard-id bits and k local bit
 * positions, ascending and paired).  local ops: 1 = 2x2 on local qubit a (m = 8 doubles), 2 = cx a -> b,
 * 3 = multiply the shard by the scalar m[0..1]. */
typedef struct qsim_shard_plan qsim_shard_plan;
typedef void (*qsim_local_op_cb)(void *user, int kind, int a, int b, const double *m);
int qsim_shard_plan_create(qsim_shard_plan **out, const qsim_circuit *circuit, int num_shards);
void qsim_shard_plan_free(qsim_shard_plan *p);
int qsim_shard_plan_num_steps(const qsim_shard_plan *p);
int qsim_shard_plan_step(const qsim_shard_plan *p, int step, int *kind, int *k, int *shard_bits, int *local_bits);
int qsim_shard_plan_final_pos(const qsim_shard_plan *p, int *pos /* num_q entries: logical -> physical */);
/* For an exchange step: where the register can be non-zero just before it, as sets of local positions / shard-id bits (a qubit
 * stays |0> until a non-diagonal gate, or a CX whose control may be 1, acts on it).  The same on every rank. */
int qsim_shard_plan_step_support(const qsim_shard_plan *p, int step, uint64_t *mixed_local, uint64_t *mixed_rank);
/* What that means for one shard in the exchange of `step` (host only; what qsim_cluster / qsim_rank_comm act on).  The shard is
 * member `mine` of its group; block b of its packed layout goes to member b and block b of its new contents comes from member b.
 * send / recv: bit b set = that block really travels (never bit `mine`); keep_own: block `mine` stays and holds data; unread:
 * blocks of the packed layout nobody looks at; empty_before / empty_after: the shard holds nothing (all zero) before / after;
 * new_support: local index bits that may be 1 in its new contents (qsim_set_support). */
typedef struct {
    int mine, empty_before, empty_after, keep_own;
    uint32_t send, recv, unread;
    uint64_t new_support;
} qsim_exchange_roles;
int qsim_shard_plan_exchange_roles(const qsim_shard_plan *p, int step, int shard, qsim_exchange_roles *out);
int qsim_shard_plan_local_ops(const qsim_shard_plan *p, int step, int shard, qsim_local_op_cb cb, void *user);
int qsim_shard_plan_apply_local(const qsim_shard_plan *p, int step, int shard, qsim_state *s);
/* Cost model of the plan's exchanges on one fully connected xGMI node: bytes each rank sends, and seconds =
 * sum over exchanges of (pack pass: 2 * shard bytes / pack_gbps) + (largest per-link transfer: 2^-k of the shard /
 * link_gbps; a k-qubit swap uses 2^k - 1 links in both directions at once).  The planner itself keeps the cheaper of
 * two placements (keep far-next-use globals vs swap all log2 P of them) under the same model with default rates. */
/* Geometry planning (qsim_tune_circuit) for one shard's local steps of the plan; leaves the shard state reset. */
int qsim_shard_plan_tune(const qsim_shard_plan *p, int shard, qsim_state *s, int max_candidates, double budget_ms, qsim_tune_report *report);
int qsim_shard_plan_predict(const qsim_shard_plan *p, double link_gbps, double pack_gbps, double *bytes_per_rank, double *seconds);

/* ---- one process per GPU: the exchanges on RCCL (pairwise ncclSend/ncclRecv of half-shards for one global
 * qubit, one group of 2^k - 1 sends + receives for k of them) ----------------------------------------------------------
 * Rank 0 calls qsim_rccl_unique_id and hands the QSIM_RCCL_ID_BYTES bytes to every rank over the launcher's own channel;
 * each rank then joins with qsim_rank_comm_create (scratch: a caller-owned device buffer as large as the shard, or NULL
 * to let the library allocate one).  qsim_rank_comm_exchange = pack kernel + ONE ncclGroup on the shard's stream, no
 * host synchronisation; qsim_rank_comm_stats reports the HIP-event time its stream spent in exchanges (measured while
 * the shard is in profile mode, QSIM_OPT_PROFILE). */
#define QSIM_RCCL_ID_BYTES 128
typedef struct qsim_rank_comm qsim_rank_comm;
int qsim_rccl_unique_id(void *id_bytes);
int qsim_rank_comm_create(qsim_rank_comm **out, qsim_state *shard, int device, int world, int rank, const void *id_bytes, void *scratch_device);
void qsim_rank_comm_destroy(qsim_rank_comm *c);
int qsim_rank_comm_exchange(qsim_rank_comm *c, const int *shard_bits, const int *local_bits, int k);
/* The exchange of step `step` of a plan, using what the plan knows about the state there (qsim_shard_plan_step_support): ranks
 * that hold nothing do not pack or send, blocks that are zero throughout are not received, and the shard's engine is told
 * where its new contents can be non-zero (qsim_set_support) or that it holds nothing (qsim_reset_shard). */
/* A plan's steps are only right in order from qsim_reset_shard (|0...0>): a rank the plan takes to hold nothing and that does hold
 * something is refused (QSIM_ERR_ARG).  Exchanges swap at most 5 qubits (groups of 32 ranks). */
int qsim_rank_comm_exchange_step(qsim_rank_comm *c, const qsim_shard_plan *p, int step);
int qsim_rank_comm_stats(qsim_rank_comm *c, uint64_t *exchanges, double *bytes_sent, double *seconds, int reset);
int qsim_rank_comm_pack_counts(const qsim_rank_comm *c, uint64_t *fused, uint64_t *separate); /* as qsim_cluster_pack_counts */
/* Diagnostic: `count` doubles of the shard through ncclSend -> ncclRecv to this same rank, compared on the host (drives
 * the RCCL call path where only one GPU is present). */
int qsim_rank_comm_loopback(qsim_rank_comm *c, uint64_t count);

int qsim_get_stats(qsim_state *s, qsim_stats *out); /* waits for outstanding profile events */
int qsim_reset_stats(qsim_state *s);
/* Test and measurement aid, not part of what the rotation call promises: rotation sweeps (qsim_apply_pauli_rotations and the
 * cluster's) launched by this process so far.  One process-wide counter for all states and shards together, which qsim_stats
 * does not have and qsim_reset_stats does not clear: take differences, and only where one thread applies rotations. */
uint64_t qsim_pauli_rotation_sweeps_launched(void);
uint64_t qsim_pauli_adjoint_sweeps_launched(void); /* the same for the backward sweeps of qsim_pauli_gradient and qsim_controlled_pauli_gradient */
/* Per-launch record (QSIM_OPT_PROFILE=1) since the last qsim_reset_stats: returns the number of records and,
 * for 0 <= index < count, fills the kernel class, the fused blocks in that launch, the tile's high-qubit
 * mask and the HIP-event time. */
long qsim_launch_log(qsim_state *s, long index, int *kernel_class, int *n_ops, uint64_t *high_mask, double *ms);
/* For a tile pass of the launch log: its high tile bits in tile-local order (order[j] = global bit of tile-local bit L+j;
 * the first three are walked by the lanes of a wave, the next by its waves, the last by a lane's registers); count = 0
 * for other kernels.  order needs room for 10 entries. */
int qsim_launch_log_order(qsim_state *s, long index, int *order, int *count);
/* ... and the fraction of the register's tiles it worked on (1 for a full sweep and for other kernels; less while the state's
 * support is partial, QSIM_OPT_SPARSE_START / qsim_set_support). */
int qsim_launch_log_visited(qsim_state *s, long index, double *visited);
/* ... and the fraction of the register it read: of a visited tile only the slots inside the state's support before the pass are
 * loaded, so this is visited / 2^(tile qubits new to the support); 0 for the pass that generates a basis state, 1 for a full
 * sweep and for other kernels.  The pass moved (visited + read_share) / 2 of the bytes of a full pass. */
int qsim_launch_log_read_share(qsim_state *s, long index, double *read_share);
/* ... and what its blocks looked like, one byte per block in order (tile passes; *count = 0 otherwise; at most `cap` are written):
 * bits 0-1 log2 of the entries per row the block is evaluated with (1, 2 or 4), bits 2-4 its qubits inside the tile, bit 5 set when
 * at least half of its rows are identity rows, bits 6-7 its selector qubits outside the tile.  Recorded under QSIM_OPT_PROFILE = 2
 * only (host work per launch).  Data for the pass-time model. */
int qsim_launch_log_blocks(qsim_state *s, long index, uint8_t *codes, int cap, int *count);
/* ... and which form of the tile kernel each of those blocks ran through, five bytes per block in the same order, copied from the
 * header of the record the kernel was given (csrc/qsim_internal.h TileOp; a cached plan keeps these bytes of its records beside
 * them, so a replayed pass reports what its first run encoded): nq (tile qubits after padding), terms (entries per row), nsel, flags and b[7] (the bits the kernel branches
 * on: log2 of terms, skipped classes, barrier between reads and writes).  codes needs room for 5 * cap bytes; *count = blocks.
 * Recorded under QSIM_OPT_PROFILE = 2 only. */
int qsim_launch_log_block_flags(qsim_state *s, long index, uint8_t *codes, int cap, int *count);

/* ---- circuits: the tokenizer of compute_state_vector (quantum_simulator.c:115-254) ---------------- */
/* Parses the OPENQASM-3 subset of quantum_simulator.c (two header statements, `qubit[n] q;` or
 * `qubit q[n];`, gates cx x sx z s sdg t tdg rz(<number>) h, operands q[k] or $k).  A file whose first
 * token is a number is read in the CUDA variants' `<num_qubit> <num_gates>` form
 * (quantum_simulator_naive.cu:239-240). */
int qsim_circuit_parse_file(const char *path, qsim_circuit **out);
int qsim_circuit_parse_text(const char *text, size_t len, qsim_circuit **out);
int qsim_circuit_create(int num_q, qsim_circuit **out);
void qsim_circuit_free(qsim_circuit *c);
int qsim_circuit_num_qubits(const qsim_circuit *c);
long qsim_circuit_num_gates(const qsim_circuit *c);
int qsim_circuit_append_1q(qsim_circuit *c, const double *U, int target);
int qsim_circuit_append_cx(qsim_circuit *c, int control, int target);
int qsim_circuit_append_2q(qsim_circuit *c, const double *U, int q_hi, int q_lo); /* q_hi > q_lo */
/* kind: QSIM_GATE_*; q0 = target / control / q_hi, q1 = -1 / target / q_lo; U receives 8 (U1) or 32 (U2) doubles */
int qsim_circuit_gate(const qsim_circuit *c, long index, int *kind, int *q0, int *q1, double *U);
/* Text of the parse error (the reference prints "Unknown token: %s", quantum_simulator.c:213). */
const char *qsim_circuit_error(void);
/* Queues gates [first, first+count) of the circuit on the state (count < 0: to the end). */
int qsim_run_circuit(qsim_state *s, const qsim_circuit *c, long first, long count);
/* The gate table (quantum_simulator.c:184-211): name -> 2x2, standard orientation. Returns QSIM_GATE_U1,
 * QSIM_GATE_CX for "cx", or 0 for an unknown token. */
int qsim_gate_matrix(const char *token, double *U);

/* ---- scheduling only (host code, no device): what a flush WOULD launch ----------------------------- */
/* Runs the fusion scheduler on a circuit and reports launches and algorithmic bytes per kernel class
 * for a state of num_q qubits at the given fuse level.  Used by tests and by the planner. */
int qsim_plan_circuit(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, qsim_stats *out);
/* The same for a run that does not start from a reset: initial_support = index bits that may be 1 in the state the circuit
 * finds (all ones: a dense state, e.g. a shard after its second exchange; 0: fresh from a reset, what qsim_plan_circuit assumes). */
int qsim_plan_circuit_from(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, uint64_t initial_support, qsim_stats *out);
/* The same schedule pass by pass (at most `cap` entries are written, *count receives the number of passes): the kernel class,
 * the blocks of a tile pass, the index bits inside its tile (all bits for a single-gate kernel), the fraction of the register it
 * visits, its algorithmic bytes and the bytes-equivalent the planning steps price it at (pass-time model).  Host-side models
 * use it to tell which passes could be pipelined beside an exchange (bench.py exchange_model). */
typedef struct {
    int32_t kernel_class, blocks;
    uint64_t tile_mask;
    double visited, bytes, cost_bytes;
} qsim_pass_info;
int qsim_plan_passes(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, uint64_t initial_support, qsim_pass_info *out, int cap, int *count);
/* The schedule qsim_schedule_circuit (defer == 0) or qsim_schedule_circuit_deferred (defer != 0) reports, for a run that finds a
 * state of the given support, with what QSIM_OPT_AFFINE_SUPPORT adds to each pass.  on: the pass is a tile pass over a partial
 * support.  The tiles it visits unless it is a closing pass (then the coordinate cube over support_before | tile_mask) are the
 * index bases origin ^ span(gen[0 .. n_gen)); refined: those are fewer than that cube.  check_mask / check_parity (bit j): the
 * region the previous pass wrote — an input index x is stale memory unless popcount(x & check_mask[j]) has parity bit j for every
 * j < n_checks.  visited / read_share: the shares of the register the pass writes and reads when it goes by its region. */
typedef struct {
    int32_t kernel_class, on, refined, n_gen, n_checks, reserved;
    uint64_t tile_mask, support_before, origin, check_parity;
    uint64_t gen[64], check_mask[64];
    double visited, read_share;
} qsim_pass_region;
int qsim_plan_regions(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support, int defer,
                      qsim_pass_region *out, int cap, int *count);
/* One candidate of the planning step (qsim_choose_schedule): the scheduler setting a schedule choice consists of.  commute < 0,
 * lookahead < 0, cheap_margin <= 0: the value the state's options give.  cap: clusters per pass (0: the options' own); seed: the
 * tie-break seed; defer: X gates left to the last pass's stores; support_weight: what a tile slot outside a partial support costs
 * the packer beyond its place (0: not weighed).  cost_bytes / is_default: filled in by qsim_plan_choice. */
typedef struct {
    int32_t commute, lookahead, cap, defer, support_weight, is_default;
    uint64_t seed;
    double cheap_margin, cost_bytes;
} qsim_sched_setting;
/* qsim_plan_regions for the level-3 schedule under a setting (its defer counts). */
int qsim_plan_regions_with(const qsim_circuit *c, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support,
                           const qsim_sched_setting *setting, qsim_pass_region *out, int cap, int *count);
/* What the pass-time model of the planning step would choose for this circuit on an fp64 (f32 != 0: fp32) state with these options
 * that has the given support, with_defer != 0: the candidates with deferred X gates take part.  out[i]: candidate i with its price
 * (at most cap are written, *count receives their number), *chosen: the index of the choice, *seconds: host time of the ranking. */
int qsim_plan_choice(const qsim_circuit *c, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support, int f32, int with_defer,
                     qsim_sched_setting *out, int cap, int *count, int *chosen, double *seconds);
/* The measured schedule choice filed under a circuit's key, as a "sched" line of the table file states it: lookup returns 1 and the
 * setting or 0; enter files one (on a device qsim_tune_circuit does). */
int qsim_sched_choice_lookup(uint64_t key, qsim_sched_setting *out);
int qsim_sched_choice_enter(uint64_t key, const qsim_sched_setting *in);
/* Same scheduler, op by op: calls `cb` for every fused block in launch order with the pass it belongs to, the
 * kernel class of that pass, the block kind (QSIM_GATE_U1 / _CX / _U2 .. _U8 by qubit count), its qubits (most
 * significant first; CX: control, target) and its matrix (2^nq x 2^nq complex, row-major; NULL for CX).  A block of a
 * tile pass may span up to 8 qubits: at most 6 inside the tile plus, listed first, at most 2 outside it in which the
 * matrix is block-diagonal (they select the sub-block a tile gets).  Lets a CPU test replay the schedule with numpy
 * and compare it with the unfused circuit. */
typedef void (*qsim_sched_cb)(void *user, int pass, int kernel_class, int kind, const int *qubits, int nq,
                              const double *U, int gates_folded);
int qsim_schedule_circuit(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops,
                          qsim_sched_cb cb, void *user);
/* The same for a run that finds a state of the given support (index bits that may be 1; 0: fresh from a reset), as
 * qsim_plan_regions with defer == 0 describes it. */
int qsim_schedule_circuit_from(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support,
                               qsim_sched_cb cb, void *user);
/* The same with the X gates deferred (QSIM_OPT_DEFER_FLIPS; level 3 only): the blocks of a schedule without them, and in *flip_mask
 * the index bits still flipped at the end — the circuit's state is the replayed one with amplitude i moved to i ^ *flip_mask.  The
 * deferred statements are counted in gates_folded of the last block reported. */
int qsim_schedule_circuit_deferred(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops,
                                   qsim_sched_cb cb, void *user, uint64_t *flip_mask);
/* The level-3 schedule under a setting (qsim_sched_setting above): its blocks, and in *flip_mask what qsim_schedule_circuit_deferred
 * reports there (0 unless the setting defers). */
int qsim_schedule_circuit_with(const qsim_circuit *c, int tile_bits, int tile_low_bits, int tile_max_ops, uint64_t initial_support,
                               const qsim_sched_setting *setting, qsim_sched_cb cb, void *user, uint64_t *flip_mask);
/* The same schedule (same arguments) as the records the tile kernel reads: `cb` is called for every block of every tile pass,
 * the tile-uniform factors included, with the pass, the geometry the record was encoded under (geom[0..2] = tile bits B, low
 * bits L, number of high bits; high[j] = global bit of tile-local bit L+j, IN ORDER), the block's qubits outside the tile
 * (selectors) and inside it (both most significant first), its matrix on (selectors..., tile qubits...) as
 * qsim_schedule_circuit reports it, and the encoded record itself (record_bytes bytes; layout: csrc/qsim_internal.h TileOp).
 * f32 != 0: the records of an fp32 state.  order_seed != 0: every pass's high bits are shuffled (seeded) before encoding, as
 * the engine may reorder them.  Host code, no device: lets a CPU test interpret the records (tests/tile_record_ref.py). */
typedef void (*qsim_tile_record_cb)(void *user, int pass, const int *geom, const int *high, const int *selectors, int nsel,
                                    const int *tile_qubits, int nq, const double *U, const void *record, long record_bytes);
int qsim_tile_records(const qsim_circuit *c, int fuse, int tile_bits, int tile_low_bits, int tile_max_ops, int f32, uint64_t order_seed,
                      qsim_tile_record_cb cb, void *user);

#ifdef __cplusplus
}
#endif
#include "qsim_qft.h"
#include "qsim_measure.h"
#endif /* QSIM_H */
