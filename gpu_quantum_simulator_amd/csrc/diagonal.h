// diagonal.h — what diagonal.hip (the kernels) and diagonal.cpp (the qsim_diagonal object, the plan, the calls) share: a real table
// d[0..2^n) of fp64 on the device as an operator on a whole register, exp(-i gamma D) and <D>, <D^2> in one sweep each,
// and the two sweeps of a gradient through such phases, the backward sweep and dst = w D src (their host side is pauli.cpp).
//
// Work is dealt in ITEMS: what one 16-byte load of the table covers, two amplitudes.  Item t = (q << kTidBits) | tid holds table
// entries 2t and 2t + 1; of the state it is two 16-byte units in fp64 and one in fp32.  Registers of fewer than 128 amplitudes
// (items < kDiagWave) take a plain path of one thread per amplitude in the same kernels: a wave of the main path moves whole blocks
// of 128 amplitudes (diagonal.hip says why), and a register of one amplitude has no 16-byte table unit at all.
#ifndef QSIM_DIAGONAL_H
#define QSIM_DIAGONAL_H

#include "pauli_sweep.h"

namespace qsim {

constexpr int kDiagWave = 64;          // items of one wave's block; fewer items than this: the plain path
constexpr int kDiagPhaseGrid = 2048;   // workgroups of a phase sweep at most (8 per CU); the resident grid where that is smaller
constexpr int kDiagTermsPerRecord = kMaxPauliTermsPerSweep; // terms one k_diag_add_terms launch adds
constexpr int kDiagAddUnitsPerTrip = 4; // table units per thread and trip of k_diag_add_terms: 8 independent chains of fp64 additions
constexpr int kDiagExtremaUnitsPerTrip = 8; // one stream, 8 loads in flight
constexpr int kDiagExtremaGrid = 1024; // workgroups of the extrema reduction at most = rows of its scratch
constexpr size_t kDiagExtremaRowDoubles = 4; // min, argmin, max, argmax (the indices as the bits of a double's 8 bytes)
constexpr size_t kDiagScratchDoubles = (size_t)(kDiagExtremaGrid + 1) * kDiagExtremaRowDoubles; // the rows, then the result

// items per thread and trip of the two sweeps over a state: about 8 independent 16-byte loads in flight.  fp64: 3 items are 9 loads
// (two state units and one table unit each; 2 would leave a quarter of the queue empty, combine.hip's choice for three streams),
// fp32: 4 items are 8 loads.  Defaults by that rule, not by measurement.
constexpr int diag_items_per_trip(bool f32) { return f32 ? 4 : 3; }
// the same rule for the sweeps over TWO states and the table (k_diag_adjoint: psi and lambda; k_diag_apply when it accumulates: src
// and dst).  An fp64 item is 5 loads, so 2 items are 10 (1 would leave three eighths of the queue empty); an fp32 item is 3 loads, so
// 3 items are 9 (2 would leave a quarter empty).  By the rule, not by measurement.
constexpr int diag_adjoint_items_per_trip(bool f32) { return f32 ? 3 : 2; }

struct DiagGeom {    // by value: a kernel argument
    uint64_t items;  // 16-byte table units to visit, 1 for a register of one amplitude
    uint64_t amps;   // amplitudes in the register = entries of the table
};
inline DiagGeom diag_geom(int n) {
    const uint64_t N = 1ULL << n;
    return DiagGeom{N < 2 ? 1 : N >> 1, N};
}

struct DiagTerms {   // by value: scalar loads
    uint64_t z[kDiagTermsPerRecord];
    double c[kDiagTermsPerRecord];
    int32_t count;
};
static_assert(sizeof(DiagTerms) <= 1024, "term records stay well inside the 4 KiB of kernel arguments");

// a_i <- exp(-i gamma d_i) a_i, gamma_over_pi = gamma / pi formed once by the host
hipError_t launch_diag_phase(const LaunchCfg &cfg, void *amps, bool f32, int n, const double *table, double gamma_over_pi);
// d_out[0] = sum_i d_i |a_i|^2, d_out[1] = sum_i d_i^2 |a_i|^2; a reducing sweep: d_partial as for launch_expect
hipError_t launch_diag_expect(const LaunchCfg &cfg, const void *amps, bool f32, int n, const double *table, double *d_partial, double *d_out);
// d_i <- (...((d_i + c_0 s_0(i)) + c_1 s_1(i)) + ...) for the record's terms, s_k(i) = (-1)^popcount(i & z_k)
hipError_t launch_diag_add_terms(hipStream_t stream, double *table, int n, const DiagTerms &terms);
// d_scratch: kDiagScratchDoubles; its last row gets min, argmin, max, argmax, ties to the lowest index
hipError_t launch_diag_extrema(hipStream_t stream, const double *table, int n, double *d_scratch);
// The backward sweep of an adjoint gradient through exp(-i gamma D): d_out[0] = sum_i d_i Im(conj(lam_i) psi_i) of the
// values as loaded, then psi_i and lam_i times exp(-i pi gamma_over_pi d_i) — one factor, formed once and rounded once.  The host
// passes gamma_over_pi = -gamma / pi: the step back.  psi != lam; a reducing sweep: d_partial as for launch_expect, cfg.grid_cap
// does not apply.
hipError_t launch_diag_adjoint(const LaunchCfg &cfg, void *psi, void *lam, bool f32, int n, const double *table, double gamma_over_pi, double *d_partial,
                               double *d_out);
// dst_i (= | +=) weight d_i src_i, out of place: src != dst; weight d_i is formed in fp64 and rounded once to the state's precision.
// Not accumulating, dst is not loaded, whatever it holds.
hipError_t launch_diag_apply(const LaunchCfg &cfg, const void *src, void *dst, bool f32, int n, const double *table, double weight, bool accumulate);

} // namespace qsim

// ---- diagonal.cpp: what other host files need of a qsim_diagonal (pauli.cpp's gradient reads tables) ------------------------------
struct qsim_state;
struct qsim_diagonal;
namespace qsim {
// QSIM_OK when both are there, over the same number of qubits and on the same device
int check_diag_pair(const char *who, const qsim_state *s, const qsim_diagonal *d);
const double *diag_table(const qsim_diagonal *d);
// Behind EVERY launch on the state's stream that reads the table: records the event a later write or add_terms waits for.
int mark_read(const qsim_state *s, const qsim_diagonal *d);
// one more in qsim_diagonal_sweeps_launched: a forward phase, an expectation value, a k_diag_apply sweep
void count_diagonal_sweep();
} // namespace qsim
#endif
