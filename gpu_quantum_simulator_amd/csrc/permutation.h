// permutation.h — what permutation.hip (the kernel) and permutation.cpp (the plan, the operand, the entry points) share: a
// permutation of the basis states of up to ten target qubits, under any number of controls, as ONE in-place sweep of the control
// subspace that moves amplitudes bit for bit.
//
// new[e | dep(perm[j])] = old[e | dep(j)] for every environment e inside the control subspace.  A TILE is a set of B index bits a
// workgroup owns at once: the k targets and the lowest index bits that are neither targets nor controls, until there are
// B = min(kPermTileBits, n - c) of them.  A tile holds every target, so it is closed under the map: the sweep is in place, a thread
// stores to the addresses it loaded, and two tiles never meet.  The walk is over AMPLITUDES in both precisions (an fp32 element is
// one 8-byte amplitude, never a 16-byte unit of two: qubit 0 may be a target), so CtrlGeom / spread are used in their fp64 shape:
// zeros = the tile bits and the controls, ones = the controls, units = the number of tiles.
//
// The operand is the tile-local destination map, one uint16 per tile-local index u (bit i of u is the i-th lowest tile bit):
// the target bits go through the caller's table, the padding bits stay.  2^B entries, at most 16 KiB.  A monomial matrix (a phase
// on each moved amplitude) would be a second table behind this one in the same scratch; nothing of it is built.
#ifndef QSIM_PERMUTATION_H
#define QSIM_PERMUTATION_H

#include "subset_sweep.h"

namespace qsim {

constexpr int kPermMaxQubits = 10;
// 64 KiB of amplitudes, the tile kernel's own sizes: 2^12 fp64 or 2^13 fp32 elements
constexpr int perm_tile_bits(bool f32) { return f32 ? 13 : 12; }
constexpr int perm_per_thread(bool f32) { return (1 << perm_tile_bits(f32)) / kTPB; } // elements and map entries a thread keeps: 16 or 32
// The default grid is the resident one, at most this many workgroups: the tile's 64 KiB of LDS let a CU hold two.  A launch never
// has more unless QSIM_OPT_GRID_CAP asks for them.
constexpr int kPermGridCap = 512;

// path 1: whole tiles of perm_tile_bits, any number of them.  path 0: n - c is below that; the one tile is the whole control subspace,
// the same kernel in its instantiation with runtime bounds, one workgroup.
struct PermutationPlan {
    int path, n, k, num_controls, tile_bits;
    bool f32;
    uint64_t mask;       // the tile's index bits
    uint64_t controls;
    uint64_t tiles;      // 2^(n - c - tile_bits)
    uint64_t units;      // 16 bytes each, read and written once: 2^(n - c) amplitudes (fp32: two to a unit; a single one counts as a unit)
    long trips_at_cap;   // tiles a workgroup walks when the grid is kPermGridCap
    int targets[kPermMaxQubits];
};
// The single place that decides.  false: k outside [0, 10] or above n, a negative control count, n outside [0, 40], a qubit outside
// [0, n) or repeated, a control among the targets, a NULL list with a positive count.
bool permutation_plan(const int *targets, int k, const int *controls, int num_controls, int n, bool f32, PermutationPlan *out);

// d_map: 2^tile_bits destinations, each below 2^tile_bits and each once.  Reads and writes the control subspace of `amps` and nothing
// else; asynchronous on cfg.stream.
hipError_t launch_permutation(const LaunchCfg &cfg, void *amps, const PermutationPlan &p, const uint16_t *d_map);

} // namespace qsim
#endif
