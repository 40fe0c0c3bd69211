// matrix.h — what matrix.hip (the kernels) and matrix.cpp (the plan, the operand, the entry points) share: a dense matrix on up to
// five target qubits, under any number of controls, as ONE in-place sweep of the control subspace on the matrix cores.
//
// psi'(., e) = U psi(., e) for every environment e inside the control subspace: a small GEMM with one column per environment.  In
// real numbers R = [Re Psi; Im Psi] has 2^(K+1) rows and R' = M R with M = [[Re U, -Im U], [Im U, Re U]], in 16 x 16 tiles of
// v_mfma_f64_16x16x4_f64: A = a 16 x 4 slice of M, B = a 4 x 16 slice of R (16 environments).  The kernel works on a SORTED subset
// of exactly K = 3, 4 or 5 qubits (fewer targets are padded as density_plan pads, with the lowest index bits that are neither
// targets nor controls, and U (x) 1 on the host) and knows nothing of Re, Im or the caller's order: the host builds M in the
// kernel's row order, and matrix_row says which (amplitude over the sorted subset, part) operand row r is.
//
// Ownership.  The instruction's maps are A[l & 15][l >> 4], B[l >> 4][l & 15], D col = l & 15, row = (l >> 4) + 4 reg.  Lane
// (e = l & 15, g = l >> 4) therefore SUPPLIES the rows r = 4 j + g of environment e (slice j of R, its row g) and RECEIVES the rows
// 16 t + 4 reg + g = 4 (4 t + reg) + g of the result: the same rows, j = 4 t + reg.  Row r = 4 j + g is labelled so that a lane's
// rows are whole 16-byte units (pauli_sweep.h): it loads each unit once, feeds its components as operand elements and stores its
// accumulators back to the same addresses — no LDS, no shuffle.  g is the two lowest unit-row bits of the subset, so one load
// instruction covers 16 consecutive environments times those bits and a wave reads whole 128-byte lines wherever the subset lies.
//
// Shapes (`mode`).  fp32 units hold two amplitudes, index bit 0 is the slot:
//   kMatrixRows  fp64, or fp32 with qubit 0 in the subset: every component of a unit is a row of R (2, or 4: the slots are two rows)
//   kMatrixEnvs  fp32, qubit 0 neither in the subset nor a control: the slots are two environments, two rounds of products per load
//   kMatrixCtrl  fp32, a control on qubit 0: only the odd slot is active, the even one is stored back as loaded
// In every fp32 shape the components are widened on load and the products are fp64 (matrix.hip says why), so M is fp64 throughout.
#ifndef QSIM_MATRIX_H
#define QSIM_MATRIX_H

#include "subset_sweep.h"

namespace qsim {

constexpr int kMatrixMaxQubits = 5;
constexpr int kMatrixMinKernelQubits = 3; // one result tile is 16 rows of R = 8 amplitudes' Re and Im
constexpr int kMatrixWaves = kTPB / 64;   // every wave walks environment blocks of its own
constexpr int kMatrixEnvsPerStep = 16;    // environment units per matrix instruction: the columns of B
enum : int { kMatrixRows = 0, kMatrixEnvs = 1, kMatrixCtrl = 2 };

constexpr int matrix_rows(int kk) { return 2 << kk; }                      // of R and of M
constexpr int matrix_slices(int kk) { return matrix_rows(kk) / 4; }        // 4-row slices of R = real rows a lane owns
constexpr int matrix_tiles(int kk) { return matrix_rows(kk) / 16; }        // 16-row tiles of the result
constexpr int matrix_components(bool f32, int mode) { return f32 && mode == kMatrixRows ? 4 : 2; } // of a unit, per round, that are rows of R
constexpr int matrix_lane_units(bool f32, int kk, int mode) { return matrix_slices(kk) / matrix_components(f32, mode); } // units a lane owns per step
constexpr int matrix_steps_per_trip(int lane_units) { return lane_units >= 4 ? 1 : 4 / lane_units; } // at least 4 independent 16-byte loads in flight
// The default grid is the resident one, at most this many workgroups (4 per CU; K = 5 keeps 64 coefficients per lane in registers
// and holds 2): the plan call reports a workgroup's trips at this cap, and a launch never has more workgroups unless
// QSIM_OPT_GRID_CAP asks for them.
constexpr int matrix_grid_cap(int kk) { return kk >= 5 ? 512 : 1024; }
// The plain path: one workgroup, every thread at most this many amplitudes of the control subspace
constexpr int kMatrixSmallPerThread = 4;

// path 0: fewer than 16 environment units, mask is the targets; units: read and written, 2^-c of the state (fp32 with a control on
// qubit 0: 2^(1-c)); env_units: the columns of the GEMM (fp32 kMatrixEnvs: two environments each); trips_at_cap: at matrix_grid_cap
struct MatrixPlan : SubsetPlan {
    int num_controls, mode;
    uint64_t controls;
    int targets[kMatrixMaxQubits];
};
// M for five qubits, the largest operand a call hands to the device (U has half as many doubles)
constexpr size_t kMatrixCoefDoubles = (size_t)matrix_rows(kMatrixMaxQubits) * matrix_rows(kMatrixMaxQubits);
// The single place that decides.  false: k outside [0, 5] or above n, a negative control count, n outside [0, 40], a qubit outside
// [0, n) or repeated, a control among the targets, a NULL list with a positive count.
bool matrix_plan(const int *targets, int k, const int *controls, int num_controls, int n, bool f32, MatrixPlan *out);

// zeros: the subset and the controls; ones: the controls (fp32: amplitude bit 0 is the slot, never inserted — first_slot says
// whether it is a control)
inline CtrlGeom matrix_geom(uint64_t subset, uint64_t controls, bool f32, int n) {
    CtrlGeom g = ctrl_geom(subset | controls, 0, f32, n);
    g.ones = controls & ~(uint64_t)(f32 ? 1 : 0);
    g.first_slot = (uint32_t)(controls & (uint64_t)(f32 ? 1 : 0));
    return g;
}

// Operand row r = 4 j + g of M and of R: *a the row of Psi (an index over the SORTED subset), *part 0 Re, 1 Im.  A lane's unit
// m = j / components has the unit-row index g + 4 m; with four components (fp32, qubit 0 in the subset) a unit is two rows of Psi.
inline void matrix_row(bool f32, int mode, int r, int *a, int *part) {
    const int g = r & 3, j = r >> 2, cr = matrix_components(f32, mode), m = j / cr, c = j % cr;
    *part = c & 1;
    *a = cr == 4 ? 2 * (g + 4 * m) + (c >> 1) : g + 4 * m;
}
// Where the lane's coefficient of (result tile t, slice s) — M[16 t + (lane & 15)][4 s + (lane >> 4)] — lies in the device copy:
// lane-major, so a wave's load of one coefficient is one run of 512 bytes
inline size_t matrix_coef_index(int kk, int t, int s, int lane) { return ((size_t)t * matrix_slices(kk) + s) * 64 + lane; }

// Path 1: d_coef holds matrix_rows^2 doubles (matrix_coef_index).  Path 0: d_coef holds U, 4^k (re, im) row-major in the caller's
// order.  Reads and writes p.units units of `amps` and nothing else; asynchronous on cfg.stream.
hipError_t launch_matrix(const LaunchCfg &cfg, void *amps, const MatrixPlan &p, const double *d_coef);

} // namespace qsim
#endif
