// subset_sweep.h — what the two sweeps over a qubit SUBSET share: density.{h,hip,cpp} (rho of the subset, read-only) and
// matrix.{h,hip,cpp} (a dense matrix on the subset under controls, in place).  Both run v_mfma_f64_16x16x4_f64 on a
// SORTED subset of 3 to 5 qubits — fewer are padded with the lowest free index bits, and the host undoes the padding — and walk
// the rest of the index through CtrlGeom / spread (pauli_sweep.h).  Here: the check of a caller's qubit list, the padding rule, the
// plan fields and probe outputs both plans have, the relation between the caller's qubit order and the sorted subset, the
// dispatch on the subset's size, and the three device helpers both kernels use.
// subsystem.{h,hip,cpp} (rho of 6 to 10 qubits in blocks and slices) borrows the list check, SubsetOrder and f64x4 and
// pads nothing; permutation.{h,hip,cpp} (a table on up to 10 qubits under controls) borrows the list check, pad_subset,
// SubsetOrder and deposit.
// NOT shared, on purpose: the kernel bodies and their shape constants (density.h, matrix.h).  The walks differ — 4 against 16
// environment units per step, g.ones, the row formula — and a shared trip loop or address table would change their instructions.
#ifndef QSIM_SUBSET_SWEEP_H
#define QSIM_SUBSET_SWEEP_H

#include "pauli_sweep.h"

namespace qsim {

// ---- the plan -------------------------------------------------------------------------------------------------------------------
// *mask = the `count` qubits of a caller's list.  false: a negative count, NULL with a positive one, a qubit outside [0, n),
// repeated, or in `taken`.  n in [0, 40] is the caller's to check.
inline bool qubit_list_mask(const int *qubits, int count, int n, uint64_t taken, uint64_t *mask) {
    if (count < 0 || (count > 0 && !qubits)) return false;
    *mask = 0;
    for (int j = 0; j < count; j++) {
        if (qubits[j] < 0 || qubits[j] >= n || ((*mask | taken) >> qubits[j] & 1ULL)) return false;
        *mask |= 1ULL << qubits[j];
    }
    return true;
}
// `subset` and the lowest index bits that are neither in it nor in `avoid`, until it has kk bits or the register of n ends
inline uint64_t pad_subset(uint64_t subset, uint64_t avoid, int kk, int n) {
    for (int q = 0; q < n && __builtin_popcountll(subset) < kk; q++)
        if (!((subset | avoid) >> q & 1ULL)) subset |= 1ULL << q;
    return subset;
}
struct SubsetPlan {      // DensityPlan and MatrixPlan add their own
    int path;            // 0: the plain one-workgroup kernel, 1: the matrix path
    int n, k, padded_k;  // padded_k: the qubits of the kernel's subset (path 0: k, nothing is padded)
    bool f32;
    uint64_t mask;       // the kernel's subset
    uint64_t units;      // 16-byte units the sweep touches
    uint64_t env_units;  // path 1: environment units
    long trips_at_cap;   // trips of a workgroup's loop when the grid is at its cap
};
inline long trips_at_cap(uint64_t steps, uint64_t per_trip, uint64_t grid_cap) {
    return (long)((steps + per_trip * grid_cap - 1) / (per_trip * grid_cap));
}
// what qsim_reduced_density_plan and qsim_apply_matrix_plan report
inline void subset_probe_outputs(const SubsetPlan &p, int *path, int *padded_k, uint64_t *kernel_mask, uint64_t *units, long *trips) {
    *path = p.path, *padded_k = p.padded_k, *kernel_mask = p.mask, *units = p.units, *trips = p.trips_at_cap;
}

// A caller's k qubits (bit j of a caller's index is qubit qubits[j]) inside the sorted subset `mask` (bit i of a subset index is
// its i-th lowest qubit): where each lies, and an index's way there and back.
struct SubsetOrder {
    uint64_t mask;
    const int *qubits; // the caller's list, which outlives this
    int k;
    int position(int j) const { return __builtin_popcountll(mask & ((1ULL << qubits[j]) - 1ULL)); } // of qubits[j] in the subset
    uint32_t to_subset(uint32_t c) const { // the padding bits 0
        uint32_t a = 0;
        for (int j = 0; j < k; j++) a |= ((c >> j) & 1u) << position(j);
        return a;
    }
    uint32_t to_callers(uint32_t a) const { // whatever the padding bits are
        uint32_t c = 0;
        for (int j = 0; j < k; j++) c |= ((a >> position(j)) & 1u) << j;
        return c;
    }
    uint32_t own() const { return to_subset((1u << k) - 1u); } // the subset-index bits that are the caller's; the rest is padding
};

// f(std::integral_constant<int, KK>{}) for the subset size KK = padded_k a kernel is instantiated for
template <typename F>
hipError_t for_subset_size(int padded_k, F &&f) {
    switch (padded_k) {
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    default: return hipErrorInvalidValue;
    }
}

// ---- device helpers -----------------------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));

// bit j of v -> the j-th lowest set bit of mask
__device__ __forceinline__ uint64_t deposit(uint32_t v, uint64_t mask) {
    uint64_t r = 0;
    for (uint64_t m = mask; m != 0; m &= m - 1ULL, v >>= 1) // uniform: the mask comes off a scalar register
        if (v & 1u) r |= m & (0ULL - m);
    return r;
}

// component c of a unit, widened; c is a constant once the loops are unrolled
__device__ __forceinline__ double pick(const double2 &v, int c) { return c == 0 ? v.x : v.y; }
__device__ __forceinline__ double pick(const float4 &v, int c) { return (double)(c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w); }

} // namespace qsim
#endif
