// measure.h — what measure.hip (the two kernels) and measure.cpp (qsim_postselect, qsim_measure, qsim_collapse_plan) share: projecting a
// state onto one outcome of k measured qubits and normalising what is left.  Two sweeps:
//     weight    W = sum |a_i|^2 over the KEPT subspace alone — the indices whose measured bits equal the outcome, 2^-k of the state —
//               read-only, walked with CtrlGeom / spread (pauli_sweep.h): `zeros` the measured positions, `ones` the outcome's bits
//     collapse  every 16-byte unit of the buffer in linear order: a unit outside the kept subspace is stored as +0.0 and never loaded,
//               a kept unit is loaded, multiplied by f = 1 / sqrt(W) and stored
// fp32: amplitude bit 0 is the slot inside a unit.  With qubit 0 measured every unit straddles the subspace: the weight counts one slot
// (CtrlGeom::first_slot / odd_slot say which), the collapse scales that slot and zeroes the other.
#ifndef QSIM_MEASURE_H
#define QSIM_MEASURE_H

#include "pauli_sweep.h"

namespace qsim {

constexpr int kCollapseUnitsPerTrip = units_per_trip(false); // 8 independent 16-byte accesses per thread and trip, in both kernels

// The kept subspace as the weight sweep walks it: ctrl_geom's insertion positions for the measured qubits, the outcome's bits as `ones`.
// fp32 with qubit 0 measured: first_slot == 1 when the kept slot is the odd one, odd_slot == 0 when it is the even one.
inline CtrlGeom collapse_weight_geom(uint64_t measured, uint64_t outcome_bits, bool f32, int n) {
    CtrlGeom g = ctrl_geom(measured, 0, f32, n);
    const uint64_t as = f32 ? 1 : 0;
    g.ones = outcome_bits & ~as;
    g.first_slot = (uint32_t)(measured & outcome_bits & as);
    g.odd_slot = (measured & as) && !(outcome_bits & as) ? 0u : 1u;
    return g;
}

struct CollapseGeom {     // k_collapse, by value: a kernel argument
    uint64_t units;       // every 16-byte unit of the buffer (one for a register of a single fp32 amplitude)
    uint64_t amps;        // amplitudes in the buffer (guards that register)
    uint64_t mask, want;  // a unit is kept when (its even amplitude index & mask) == want; fp32: without bit 0
    uint32_t slot_measured, slot_kept; // fp32, qubit 0 measured: the slot that is scaled; the other one is zeroed
};
inline CollapseGeom collapse_geom(uint64_t measured, uint64_t outcome_bits, bool f32, int n) {
    const uint64_t N = 1ULL << n, as = f32 ? 1 : 0;
    CollapseGeom g{};
    g.units = N >> as ? N >> as : 1;
    g.amps = N;
    g.mask = measured & ~as, g.want = outcome_bits & ~as;
    g.slot_measured = (uint32_t)(measured & as), g.slot_kept = (uint32_t)(outcome_bits & as);
    return g;
}

// measured: the measured qubits as a mask inside the register of n, outcome_bits: the outcome deposited on them (a subset of measured).
// d_out[0] = W.  A reducing sweep: d_partial as for launch_expect, cfg.grid_cap does not apply.
hipError_t launch_collapse_weight(const LaunchCfg &cfg, const void *amps, bool f32, int n, uint64_t measured, uint64_t outcome_bits, double *d_partial,
                                  double *d_out);
// a_i <- f a_i inside the kept subspace (the fp64 product rounded once to the state's precision), +0.0 outside it
hipError_t launch_collapse(const LaunchCfg &cfg, void *amps, bool f32, int n, uint64_t measured, uint64_t outcome_bits, double f);
// the workgroups of the two sweeps at their caps when the occupancy query gives nothing smaller: what qsim_collapse_plan's trips go by
constexpr int kCollapseWeightGridCap = kExpectGrid, kCollapseGridCap = 1024;

} // namespace qsim
#endif
