/*
 * qsim_measure.h — projective measurement on the device: post-selection, measurement by a draw, the plan probe.
 * Part of the C ABI of libqsim.so: qsim.h pulls this file in with one #include line, and a program includes qsim.h, never this.
 *
 * A header of its own keeps one feature's declarations and contract in one place; its ctypes signatures are _lib.MEASURE_SIGNATURES.
 * The lazy-state census (tests/test_lazy_cases_cpu.py) follows the #include "qsim_*.h" lines of qsim.h, so a call declared here that
 * takes a qsim_state needs its entry in tests/lazy_cases.py like any other: qsim_postselect and qsim_measure open with settle() and
 * have their cases there, which tests/test_gpu_lazy_states.py runs from every lazy start over poisoned memory against a dense twin,
 * bit for bit.
 */
#ifndef QSIM_MEASURE_H_ABI
#define QSIM_MEASURE_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Projects the state onto `outcome` of the k qubits `qubits` (distinct, any order and places; bit j of the outcome is qubits[j];
 * k in [0, n], outcome < 2^k) and normalises what is left: every amplitude whose measured bits differ from the outcome becomes +0.0,
 * every other one is multiplied by 1 / sqrt(W), W = the sum of |a_i|^2 over the kept amplitudes, which *weight receives.  Afterwards
 * the squared norm is 1 whatever it was before; k == 0 normalises the state.
 * The call settles the state first (queued gates are launched, a lazily held state is written out) and does not go through the gate
 * queue.  Two sweeps: a read-only one over the kept 2^-k of the state for W (fp64 sums in both precisions, added in a fixed order:
 * equal bits whatever QSIM_OPT_GRID_CAP is), one synchronisation of the state's stream to bring W to the host, and one that writes the
 * whole buffer — it stores the discarded amplitudes WITHOUT loading them, so whatever memory holds there is never looked at — launched
 * and not waited for.  The factor is formed once in fp64 and every product is rounded once to the state's precision; each amplitude is
 * written by one thread.  The sweeps are NOT counted in the qsim_stats record; qsim_collapse_sweeps_launched counts them.
 * QSIM_ERR_ARG, no bit of the state changed: W is zero or not finite ("outcome has probability zero": only the weight sweep ran, and
 * *weight holds W), a state that holds nothing (qsim_holds_nothing; nothing is launched), and — nothing launched — a NULL argument,
 * qubits NULL with k > 0, k outside [0, n], a qubit outside the register or repeated, outcome >= 2^k.
 * Single states only, fp64 and fp32: there is NO cluster counterpart. */
int qsim_postselect(qsim_state *s, const int *qubits, int k, uint64_t outcome, double *weight);
/* Measures the k qubits: *outcome is EXACTLY what qsim_sample_shots returns for one shot on the same state, the same qubits and
 * the same draw in [0, 1] — the call runs that sampler (its pyramid, one draw), not one of its own — and the state is then collapsed
 * onto it by the two sweeps of qsim_postselect.  *probability = W / T, T being the sampler's total: an unnormalised state measures
 * |a|^2 / norm2, as the sampler draws.  k == 0: outcome 0, probability 1 up to rounding, the state normalised.
 * QSIM_ERR_ARG as above, and for a draw outside [0, 1] or not a number, and a state whose total probability is zero or not finite. */
int qsim_measure(qsim_state *s, const int *qubits, int k, double draw, uint64_t *outcome, double *probability);
/* Host only, no device: what the two sweeps walk on a register of num_q qubits held in precision_bits (64 or 32).  *weight_units:
 * 16-byte units the weight sweep reads (fp64 2^(n-k); fp32 half as many, but as many when qubit 0 is measured: one slot of every unit
 * counts; never below 1); *collapse_units: units the collapse sweep writes (the whole buffer: fp64 2^n, fp32 2^(n-1), never below 1);
 * *weight_trips, *collapse_trips: trips of a workgroup's loop — 256 threads, 8 units each per trip — at the caps of the two grids,
 * 1024 workgroups each.  QSIM_ERR_ARG: the list and outcome refusals above, num_q outside [0, 40], precision_bits other than 64 or
 * 32, a NULL result pointer. */
int qsim_collapse_plan(const int *qubits, int k, uint64_t outcome, int num_q, int precision_bits, uint64_t *weight_units, uint64_t *collapse_units,
                       long *weight_trips, long *collapse_trips);
uint64_t qsim_collapse_sweeps_launched(void); /* process-wide: + 2 per accepted qsim_postselect or qsim_measure, + 0 per refused one */

#ifdef __cplusplus
}
#endif
#endif
