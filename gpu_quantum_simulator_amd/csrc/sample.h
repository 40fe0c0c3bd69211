// sample.h — what sample.hip (the kernels) and sample.cpp (qsim_sample_geometry, qsim_sample_shots) share: drawing basis states of a
// whole register on the device.  The cumulative distribution of |a_i|^2 is never written at amplitude resolution; what
// is kept is a pyramid of three levels:
//     chunk   2^cb amplitudes, cb = min(8, n): what one wave scans (four trips of 64 amplitudes)
//     group   2^gb amplitudes, gb = min(18, n): at most 1024 chunks
//     top     one entry per group
// W[g * chunks_per_group + c] is the running sum of the chunk totals inside group g, T[g] the running sum of the group totals; both are
// SEQUENTIAL sums of non-negative terms, so they are monotone and can be bisected.  All sums are fp64 in both precisions.
#ifndef QSIM_SAMPLE_H
#define QSIM_SAMPLE_H

#include "pauli_sweep.h"

namespace qsim {

constexpr int kSampleChunkBits = 8;   // cb at most: 256 amplitudes
constexpr int kSampleGroupBits = 18;  // gb at most: 1024 chunks
constexpr int kSampleTrips = (1 << kSampleChunkBits) / 64; // trips of one wave over a chunk
constexpr int kSampleWaves = kTPB / 64;                    // waves of a workgroup of k_sample_chunk_sums and k_sample_draws: a chunk or a draw each
constexpr int kSamplePrefixTile = 1 << (kSampleGroupBits - kSampleChunkBits); // entries one wave of k_sample_prefix stages through LDS: a group's chunks
constexpr int kSampleGrid = 2048;     // workgroups of the chunk sweep and of the draws at most (8 per CU); the resident grid where that is smaller
constexpr int kSampleMaxQubits = 64;  // bits of an outcome

struct SampleGeom {       // by value: a kernel argument
    uint64_t amps;        // amplitudes in the register
    uint64_t chunks;      // 2^(n - cb): entries of W
    uint64_t groups;      // 2^(n - gb): entries of T
    int32_t chunk_bits;   // cb
    int32_t group_chunk_bits; // gb - cb: log2 chunks per group
};
inline SampleGeom sample_geom(int n) {
    const int cb = n < kSampleChunkBits ? n : kSampleChunkBits, gb = n < kSampleGroupBits ? n : kSampleGroupBits;
    return SampleGeom{1ULL << n, 1ULL << (n - cb), 1ULL << (n - gb), cb, gb - cb};
}
// bytes of W and T together: what a call allocates besides its draws and results
inline uint64_t sample_scratch_bytes(const SampleGeom &g) { return 8 * (g.chunks + g.groups); }

struct SampleQubits {     // by value: scalar loads.  count == 0: the result is the basis index itself
    uint8_t q[kSampleMaxQubits]; // bit j of an outcome is bit q[j] of the index
    int32_t count;
};

// d_w[c] = the total of chunk c: the last value of chunk_scan over it.  One read-only sweep of the state.
hipError_t launch_sample_chunk_sums(const LaunchCfg &cfg, const void *amps, bool f32, int n, double *d_w);
// d_w -> W in place (one sequential chain per group), d_t[g] = T[g] (one sequential chain over the groups' last W)
hipError_t launch_sample_prefix(const LaunchCfg &cfg, int n, double *d_w, double *d_t);
// d_out[k] = the index (or the outcome on `qubits`) of draw d_draws[k] in [0, 1], scaled by the state's own total T[last] > 0
hipError_t launch_sample_draws(const LaunchCfg &cfg, const void *amps, bool f32, int n, const double *d_w, const double *d_t, const double *d_draws,
                               long shots, const SampleQubits &qubits, uint64_t *d_out);

} // namespace qsim
#endif
