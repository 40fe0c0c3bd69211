// measure.hip — the two sweeps of a projective measurement (gfx950): the weight of one outcome of k measured qubits, and the collapse
// onto it with the normalisation folded in (measure.h has the rule, measure.cpp the calls).  Its own object, like the Pauli
// sweeps: nothing here is compiled into kernels.hip.  No LDS beyond the four doubles of the block reduction's hand-over, no atomics.
//
// k_collapse_weight reads the kept subspace alone: a unit index becomes an amplitude index by inserting a zero at every measured
// position, lowest first (spread), and OR-ing the outcome's bits in.  As in k_pauli_crot the expansion is linear over OR: E(q0 <<
// kTidBits) is uniform over the workgroup, E(u << kTidBits) is formed before the loop and E(tid) is the thread's own.  fp64: a measured
// qubit below bit 3 thins the 128-byte lines, it does not break them up.  Sums are fp64 in both precisions (a float's square is exact
// there); reduction: k_combine's — one chain per thread, wave butterfly, waves added in order, one row per workgroup,
// launch_expect_final — on reducing_grid, so W has equal bits whatever QSIM_OPT_GRID_CAP says.
//
// k_collapse walks every unit of the buffer in linear order, consecutive lanes on consecutive units.  Whether a unit is kept is a
// compare of its index; the load sits under that compare, so a discarded unit costs a 16-byte store of zeros and no read — what is in
// memory there (NaN, Inf) never reaches a register.  Where the lowest measured qubit is at or above unit bit 11 a whole workgroup trip is
// stores only.  Every amplitude is written by exactly one thread: equal calls give equal bits whatever the grid.
#include "measure.h"

namespace qsim {
namespace {

constexpr int U = kCollapseUnitsPerTrip;
static_assert((U & (U - 1)) == 0, "q0 is a multiple of U: E(q0 + u) = E(q0) | E(u)");

template <typename R>
__global__ __launch_bounds__(kTPB) void k_collapse_weight(const R *__restrict__ a, CtrlGeom g, uint64_t amps, double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2; // amplitudes per unit
    const uint32_t tid = threadIdx.x;
    const bool tiny = A == 2 && amps < 2;     // a register of one fp32 amplitude is 8 bytes long
    const uint64_t jl = spread<R>(g, tid) | g.ones;
    uint64_t eu[U];
#pragma unroll
    for (int u = 0; u < U; u++) eu[u] = spread<R>(g, (uint64_t)u << kTidBits);
    // fp32: the slots that count (both, unless qubit 0 is measured)
    const bool even = A == 1 || g.first_slot == 0, odd = A == 2 && g.odd_slot != 0 && !tiny;

    double acc = 0.0;
    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.units; q0 += (uint64_t)gridDim.x * U) {
        const uint64_t j0 = spread<R>(g, q0 << kTidBits);
        V v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            v[u] = V{};
            if (t < g.units) {
                if constexpr (A == 2) {
                    if (tiny) {
                        const float2 one = *reinterpret_cast<const float2 *>(a);
                        v[u].x = one.x, v[u].y = one.y;
                        continue;
                    }
                }
                v[u] = load_unit(a, j0 | eu[u] | jl);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) { // a unit past the end was left zero and adds +0.0
            if constexpr (A == 1) {
                acc += fma(v[u].x, v[u].x, v[u].y * v[u].y);
            } else {
                const double r0 = v[u].x, i0 = v[u].y, r1 = v[u].z, i1 = v[u].w;
                if (even) acc += fma(r0, r0, i0 * i0);
                if (odd) acc += fma(r1, r1, i1 * i1);
            }
        }
    }

    __shared__ double part[kTPB / 64];
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < kTPB / 64; w++) s += part[w];
        partial[blockIdx.x] = s;
    }
}

template <typename R>
__global__ __launch_bounds__(kTPB) void k_collapse(R *a, CollapseGeom g, double f) {
    using V = typename Vec16<R>::type;
    constexpr int AS = sizeof(R) == 8 ? 0 : 1; // log2 amplitudes per unit
    const uint32_t tid = threadIdx.x;
    if constexpr (AS == 1) {
        if (g.amps < 2) { // one fp32 amplitude, 8 bytes: nothing can be measured there, the outcome is the empty one
            if (blockIdx.x == 0 && tid == 0) {
                const float2 one = *reinterpret_cast<const float2 *>(a);
                *reinterpret_cast<float2 *>(a) = float2{(float)((double)one.x * f), (float)((double)one.y * f)};
            }
            return;
        }
    }
    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.units; q0 += (uint64_t)gridDim.x * U) {
        V v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            v[u] = V{};
            if (t < g.units && (((t << AS) & g.mask) == g.want)) v[u] = *reinterpret_cast<const V *>(a + 2 * (t << AS));
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            if (t >= g.units) continue;
            V out{}; // +0.0 in every component
            if (((t << AS) & g.mask) == g.want) {
                if constexpr (AS == 0) {
                    out = V{v[u].x * f, v[u].y * f};
                } else {
                    const bool lo = !g.slot_measured || g.slot_kept == 0, hi = !g.slot_measured || g.slot_kept == 1;
                    if (lo) out.x = (float)((double)v[u].x * f), out.y = (float)((double)v[u].y * f);
                    if (hi) out.z = (float)((double)v[u].z * f), out.w = (float)((double)v[u].w * f);
                }
            }
            *reinterpret_cast<V *>(a + 2 * (t << AS)) = out;
        }
    }
}

template <typename R>
hipError_t launch_weight_prec(const void *amps, const CtrlGeom &g, uint64_t N, hipStream_t stream, double *d_partial, double *d_out) {
    const unsigned grid = reducing_grid<k_collapse_weight<R>>(g.units, (uint64_t)kTPB * U);
    hipLaunchKernelGGL((k_collapse_weight<R>), dim3(grid), dim3(kTPB), 0, stream, (const R *)amps, g, N, d_partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_expect_final(stream, d_partial, (int)grid, 1, d_out);
}

template <typename R>
hipError_t launch_collapse_prec(const LaunchCfg &cfg, void *amps, const CollapseGeom &g, double f) {
    unsigned grid = writing_grid<k_collapse<R>>(cfg, g.units, (uint64_t)kTPB * U);
    if (cfg.grid_cap <= 0 && grid > (unsigned)kCollapseGridCap) grid = (unsigned)kCollapseGridCap;
    hipLaunchKernelGGL((k_collapse<R>), dim3(grid), dim3(kTPB), 0, cfg.stream, (R *)amps, g, f);
    return hipGetLastError();
}

bool masks_fit(uint64_t measured, uint64_t outcome_bits, int n) {
    return n >= 0 && n <= 40 && measured < (1ULL << n) && (outcome_bits & ~measured) == 0;
}

} // namespace

hipError_t launch_collapse_weight(const LaunchCfg &cfg, const void *amps, bool f32, int n, uint64_t measured, uint64_t outcome_bits, double *d_partial,
                                  double *d_out) {
    if (!amps || !d_partial || !d_out || !masks_fit(measured, outcome_bits, n)) return hipErrorInvalidValue;
    const CtrlGeom g = collapse_weight_geom(measured, outcome_bits, f32, n);
    return f32 ? launch_weight_prec<float>(amps, g, 1ULL << n, cfg.stream, d_partial, d_out)
               : launch_weight_prec<double>(amps, g, 1ULL << n, cfg.stream, d_partial, d_out);
}

hipError_t launch_collapse(const LaunchCfg &cfg, void *amps, bool f32, int n, uint64_t measured, uint64_t outcome_bits, double f) {
    if (!amps || !masks_fit(measured, outcome_bits, n)) return hipErrorInvalidValue;
    const CollapseGeom g = collapse_geom(measured, outcome_bits, f32, n);
    return f32 ? launch_collapse_prec<float>(cfg, amps, g, f) : launch_collapse_prec<double>(cfg, amps, g, f);
}

} // namespace qsim
