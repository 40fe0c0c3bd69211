/*
 * qsim_qft.h — the quantum Fourier transform on any qubits of a state, one sweep per digit of at most ten bits.
 * Part of the C ABI of libqsim.so: qsim.h pulls this file in with one #include line, and a program includes qsim.h, never this.
 *
 * A header of its own keeps one feature's declarations and contract in one place; its ctypes signatures are _lib.QFT_SIGNATURES.
 * The lazy-state census (tests/test_lazy_cases_cpu.py) follows the #include "qsim_*.h" lines of qsim.h, so a call declared here that
 * takes a qsim_state needs its entry in tests/lazy_cases.py like any other: qsim_apply_qft opens with settle() and has its cases there
 * (an in-place one and a moving one), which tests/test_gpu_lazy_states.py runs from every lazy start over poisoned memory against a
 * dense twin, bit for bit.
 */
#ifndef QSIM_QFT_H_ABI
#define QSIM_QFT_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* For every environment e (the index bits outside the k qubits)
 *     new[e | dep(y)] = 2^(-k/2) sum_x exp(+ 2 pi i x y / 2^k) old[e | dep(x)],      inverse != 0: exp(- ...),
 * dep putting bit j of its argument on qubit qubits[j] (qubits[0] = LSB, any order, any places: the convention of
 * qsim_apply_permutation).  The output is in natural order: the textbook circuit with its final swaps.  k in [0, n], the whole
 * register included; k == 0 is accepted and does nothing.
 * The call settles the state first (queued gates are launched, a lazily held state is written out) and launches its sweeps on the
 * state's stream without waiting.  It does not go through the gate queue.  The register splits into digits of at most
 * max_digit_bits bits (0: the plan's own choice; 1 ... 10: a cap, for tests and tuning) and every digit is one sweep that reads and
 * writes the whole state once: the DFT over the digit inside a 64 KiB tile in shared memory, butterflies in registers, the twiddle
 * factors towards the remaining digits (formed in fp64 from an exact fraction, rounded once to the state's precision) in the stores.
 * A sweep that is not the last moves the remaining digits up and so writes a second buffer: the idle spare buffer
 * (qsim_set_spare_buffer), else one the state allocates on first use and keeps.  The sweeps that write the other buffer are even in
 * number, so the state ends in the buffer it started in: qsim_device_ptr and an external buffer stay valid.  k <= the cap: one sweep,
 * in place, no second buffer.  Each amplitude is formed by one thread in a fixed order: equal calls give equal bits whatever
 * QSIM_OPT_GRID_CAP is.  Sweeps are NOT counted in the qsim_stats record; qsim_qft_sweeps_launched counts them, the plan's *passes per
 * accepted call.  A shard that holds nothing (qsim_holds_nothing) stays as it is and launches no sweep.
 * QSIM_ERR_ARG, nothing launched and no bit changed: a NULL state, qubits NULL with k > 0, k outside [0, n], a qubit outside the
 * register or repeated, max_digit_bits outside [0, 10].  QSIM_ERR_ALLOC, the state's bits left alone: no second buffer can be had.
 * Single states only, fp64 and fp32: there is NO cluster counterpart.  Out of scope: controls, a bit-reversed output. */
int qsim_apply_qft(qsim_state *s, const int *qubits, int k, int inverse, int max_digit_bits);
int qsim_apply_qft_max_digit_bits(void); /* 10 */
/* Host only, no device: what the call above does on a register of num_q qubits held in precision_bits (64 or 32).  *passes sweeps
 * (0 for k == 0); for sweep p < *passes digit_bits[p] (their sum is k, each at most the cap), out_of_place[p] (1: it writes the other
 * buffer; an even number of them) and tile_mask[p] (the digit's qubits and the lowest index bits outside them, min(12 | 13, n) in
 * all) — arrays of 40 each; *tiles and *units per sweep (2^(n - B) tiles; 16-byte units read and written once: fp64 2^n, fp32 half
 * as many, never below 1); *trips_per_workgroup: the tiles a workgroup walks at the default grid's cap of 512 workgroups.
 * QSIM_ERR_ARG as above, and for num_q outside [0, 40], precision_bits other than 64 or 32, a NULL result pointer. */
int qsim_apply_qft_plan(const int *qubits, int k, int num_q, int precision_bits, int max_digit_bits, int *passes, int *digit_bits,
                        int *out_of_place, uint64_t *tile_mask, uint64_t *tiles, uint64_t *units, long *trips_per_workgroup);
uint64_t qsim_qft_sweeps_launched(void); /* process-wide counter, as qsim_density_sweeps_launched */

#ifdef __cplusplus
}
#endif
#endif
