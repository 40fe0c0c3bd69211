// density.h — what density.hip (the kernels) and density.cpp (the plan, the entry points, the way from tiles to rho) share:
// reduced density matrices rho_A = Tr_B |psi><psi| of up to five qubits from ONE read-only sweep.
//
// rho = Psi Psi^+ with Psi the 2^k x 2^(n-k) matrix of amplitudes (row: the subset's bits, column: the environment).  With the real
// matrix R = [Re Psi; Im Psi] of 2^(k+1) rows, G = R R^T holds it all: Re rho = G_RR + G_II, Im rho = G_IR - G_RI.  G is
// accumulated in 16x16 tiles by v_mfma_f64_16x16x4_f64, four environments per instruction; symmetric, so only the tiles (s, t) with
// s <= t exist.  The kernel works on a SORTED subset of exactly 3, 4 or 5 qubits (fewer are padded, the host traces the padding
// out) and knows nothing of Re, Im or the caller's order: it multiplies operand tiles, and density_row() says which row of R lane
// row i of operand tile `tile` is.
//
// Shapes.  A lane loads 16-byte units (pauli_sweep.h): one fp64 amplitude, two fp32 amplitudes — index bit 0 is the slot.  Per shape
//   fp64                      2^k row units, 2 components (Re, Im) that are rows of R
//   fp32, qubit 0 outside     2^k row units, 2 components per slot; the two slots are two environments: two rounds per load
//   fp32, qubit 0 inside      2^(k-1) row units, 4 components (Re even row, Im even, Re odd, Im odd), all rows of R
// Lane l works on row unit (l & 15) and environment unit e0 + (l >> 4).  16 row units or more: load t of a step covers row units
// 16 t + i and component c of it is operand tile c * loads + t.  Fewer (8 or 4): one load, the row unit is i mod units, and lane row
// i takes component tile * (16 / units) + i / units — 16 / units lanes load the same unit.
#ifndef QSIM_DENSITY_H
#define QSIM_DENSITY_H

#include "subset_sweep.h"

namespace qsim {

constexpr int kDensityMaxQubits = 5;
constexpr int kDensityMinKernelQubits = 3; // one operand tile is 16 rows of R = 8 amplitudes' Re and Im
constexpr int kDensityWaves = kTPB / 64;   // every wave walks environment blocks of its own

constexpr int density_row_units(bool f32, int kk, bool q0_in) { return f32 && q0_in ? 1 << (kk - 1) : 1 << kk; }
constexpr int density_components(bool f32, bool q0_in) { return f32 && q0_in ? 4 : 2; }   // of a unit, that are rows of R
constexpr int density_env_slots(bool f32, bool q0_in) { return f32 && !q0_in ? 2 : 1; }   // environments in one unit
constexpr int density_loads(int row_units) { return row_units >= 16 ? row_units / 16 : 1; } // per lane and step
constexpr int density_steps_per_trip(int loads) { return 8 / loads; }                      // 8 independent 16-byte loads in flight
constexpr int density_tiles(int kk) { return (2 << kk) / 16; }                             // operand tiles = rows of R / 16
constexpr int density_upper_tiles(int kk) { return density_tiles(kk) * (density_tiles(kk) + 1) / 2; }
constexpr int density_row_doubles(int kk) { return density_upper_tiles(kk) * 256; }         // one partial row = one result

// path 0: registers too small for a tile; units: the state, read once; env_units: units per row unit; trips_at_cap: at kExpectGrid
struct DensityPlan : SubsetPlan {
    bool q0_in; // qubit 0 is in the kernel's subset
};
// The single place that decides.  false: k outside [0, 5] or above n, n outside [0, 40], a qubit outside [0, n) or repeated.
bool density_plan(const int *qubits, int k, int n, bool f32, DensityPlan *out);

// Row of R behind lane row i (0..15) of operand tile `tile`: *part 0 Re, 1 Im; *a the row of Psi (an index over the SORTED subset).
inline void density_row(const DensityPlan &p, int tile, int i, int *part, int *a) {
    const int ru = density_row_units(p.f32, p.padded_k, p.q0_in), loads = density_loads(ru);
    int c, m;
    if (ru >= 16) c = tile / loads, m = 16 * (tile % loads) + i;
    else c = tile * (16 / ru) + i / ru, m = i % ru;
    if (p.f32 && p.q0_in) *part = c & 1, *a = 2 * m + (c >> 1);
    else *part = c, *a = m;
}
// Where element (i, j) of tile (s, t), s <= t — the s-th operand tile times the transposed t-th — lies in a result row:
// C/D of the fp64 matrix instruction has col = lane & 15, row = (lane >> 4) + 4 reg.
inline int density_tile_index(int tiles, int s, int t) { return s * tiles - s * (s - 1) / 2 + (t - s); }
inline int density_element(int tiles, int s, int t, int i, int j) {
    return (density_tile_index(tiles, s, t) * 4 + (i >> 2)) * 64 + ((i & 3) << 4 | j);
}

// Doubles of device scratch a sweep needs: kExpectGrid partial rows and the result row behind them (path 0: the result alone).
size_t density_scratch_doubles(const DensityPlan &p);
// Path 1: the result row (density_row_doubles) at d_scratch + kExpectGrid rows.  Path 0: rho over the sorted subset, 4^k (re, im)
// row-major at d_scratch.  Reads p.units units of `amps` and nothing else; asynchronous on cfg.stream, cfg.grid_cap does not apply.
hipError_t launch_density(const LaunchCfg &cfg, const void *amps, const DensityPlan &p, double *d_scratch);
inline double *density_result(const DensityPlan &p, double *d_scratch) {
    return p.path ? d_scratch + (size_t)kExpectGrid * density_row_doubles(p.padded_k) : d_scratch;
}

} // namespace qsim
#endif
