// subsystem.h — what subsystem.hip (the kernels) and subsystem.cpp (the plan, the entry points, the way from blocks to rho) share:
// reduced density matrices of 6 to 10 qubits, G = R R^T cut into blocks and slices.  Five qubits and fewer stay with
// density.{h,hip,cpp} (§7h), whose result fits one wave.
//
// rho = Psi Psi^+ with Psi the 2^k x 2^(n-k) matrix of amplitudes (row: the SORTED subset's bits, column: the environment), and
// G = R R^T for the real matrix R of M = 2^(k+1) rows as in §7h.  Here the rows of R are interleaved, row 2 a is Re Psi[a] and row
// 2 a + 1 is Im Psi[a], so that a 16-byte unit of the state is two neighbouring rows of R (fp64) and a block of B consecutive rows
// of R is B / 2 consecutive rows of Psi with both their parts.
//   Blocks.  G is cut into square blocks of B = 128 rows; block row b holds the rows of Psi with a >> 6 == b.  Only the blocks
//     (bi, bj) with bi <= bj are computed, numbered row by row (subsystem_block_index); of a diagonal block, which is symmetric
//     itself, only the 16 x 16 tiles with row <= column, the others are zeros.
//   Slices.  The 2^(n-k) environments come in chunks of E = 32 consecutive environment indices (fewer when the register has fewer);
//     slice s is the chunks [s T, (s + 1) T), T = chunks / S.  One workgroup takes one (block, slice): per chunk it stages the panel
//     of bi (128 rows x E environments, widened to fp64) and, off the diagonal, the panel of bj in LDS, and its four waves multiply
//     a 64 x 64 quarter each, 16 accumulator tiles of v_mfma_f64_16x16x4_f64 per wave (a diagonal block: 9 of its 36 tiles each;
//     the two kinds of block are two instantiations of the kernel, launched one after the other).  It writes its block, row-major,
//     to partial (s, block); k_subsystem_final adds the S partials of every element in ascending slice order.  No atomics.
//   B, E, S and the order are functions of (n, k, precision, subset) alone: equal calls return equal bits on any device.
#ifndef QSIM_SUBSYSTEM_H
#define QSIM_SUBSYSTEM_H

#include "subset_sweep.h"

namespace qsim {

constexpr int kSubsystemMaxQubits = 10;   // beyond: the 4^k result and its diagonalisation on the host dominate the call
constexpr int kSubsystemMinQubits = 6;    // fewer: qsim_reduced_density
constexpr int kSubBlockRows = 128;        // B: rows of R in a block = 64 rows of Psi
constexpr int kSubBlockAmpBits = 6;       // log2(B / 2)
constexpr int kSubChunkEnvBits = 5;       // E = 32 environments per chunk
constexpr int kSubPanelStride = kSubBlockRows + 16; // doubles between two environments of a panel in LDS: lanes (i, e) and (i, e + 1)
                                                    // of a ds_read_b64 half fall 16 double slots apart, so the half covers all 64 banks
constexpr int kSubPanelDoubles = (1 << kSubChunkEnvBits) * kSubPanelStride;
constexpr long kSubMaxPartialBlocks = 4096; // S * upper blocks at most: 512 MiB of partial blocks
constexpr long kSubMaxSlices = 1024;
constexpr int kSubMinTrips = 4;           // a workgroup walks at least this many chunks where the register has them
constexpr int kSubPlainGrid = 1024;       // workgroups of the plain kernel at most

struct SubsystemPlan {
    int path;              // 0: the plain kernel (n - k < 2), 1: blocks and slices
    int n, k;
    bool f32;
    uint64_t mask;         // the subset
    int block_rows;        // B; path 0: 0
    long blocks;           // block rows of G: M / B
    long upper_blocks;     // blocks * (blocks + 1) / 2; path 0: 0
    int chunk_env_bits;    // log2 of the environments in a chunk: min(5, n - k)
    long chunks, slices, trips; // chunks = slices * trips; path 0: 0, 0, 1
    uint64_t units_read;   // 16-byte units loaded by all workgroups together
    uint64_t scratch_bytes;
};
// The single place that decides.  false: k outside [0, 10] or above n, n outside [0, 40], a qubit outside [0, n) or repeated.
// (k <= 5 is planned too, as path 0 or 1 of THIS file's kernels would run it; the entry point forwards those to qsim_reduced_density.)
bool subsystem_plan(const int *qubits, int k, int n, bool f32, SubsystemPlan *out);

inline long subsystem_block_index(long blocks, long bi, long bj) { return bi * blocks - bi * (bi - 1) / 2 + (bj - bi); }
constexpr size_t kSubBlockDoubles = (size_t)kSubBlockRows * kSubBlockRows;
// Path 1: partial (s, block) at d_scratch + (s * upper_blocks + block) * B^2, the result blocks behind the last partial.
// Path 0: rho over the sorted subset, 4^k (re, im) row-major, at d_scratch.
inline double *subsystem_result(const SubsystemPlan &p, double *d_scratch) {
    return p.path ? d_scratch + (size_t)p.slices * p.upper_blocks * kSubBlockDoubles : d_scratch;
}
// Reads the state and nothing else, writes p.scratch_bytes at d_scratch; asynchronous on the stream.
hipError_t launch_subsystem(hipStream_t stream, const void *amps, const SubsystemPlan &p, double *d_scratch);
// `instructions` v_mfma_f64_16x16x4_f64 per wave (rounded to whole rounds of 128) on registers alone, 16 independent accumulator
// tiles as in the sweep, in `workgroups` workgroups of four waves that reserve lds_bytes each; *ms: the second of two runs, by
// events on the null stream.  The bench's arithmetic yardstick.
hipError_t launch_mfma_probe(long instructions, int workgroups, int lds_bytes, float *ms);

} // namespace qsim
#endif
