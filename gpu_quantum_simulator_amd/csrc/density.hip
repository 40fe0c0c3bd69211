// density.hip — reduced density matrices of up to five qubits as ONE read-only sweep on the matrix cores (gfx950).  Its own object,
// like the Pauli sweeps: nothing here is compiled into kernels.hip.  density.h has the decomposition (rho from G = R R^T, the
// shapes, which row of R a lane row is), subset_sweep.h what matrix.hip uses too, and density.cpp the host side; this file has the two kernels.
//
// k_density (the matrix path).  A wave works on its own: lane l loads the unit of (row unit l & 15, environment unit e0 + (l >> 4)),
// and a component of that unit IS the lane's element of an operand of v_mfma_f64_16x16x4_f64 — A[l & 15][l >> 4] and B[l >> 4][l & 15]
// are the same register, so the tile (s, t) of G is mfma(op[s], op[t]) with no LDS and no shuffle; fp32 components are widened
// first, so every product is exact and every sum is fp64.  The environment index is expanded to an amplitude index by inserting
// zeros at the subset's bits (spread: zeros = the subset, no ones).  A wave takes U consecutive steps of four environment units per
// trip, all loads first: with the subset on high bits one load instruction touches 16 runs of 64 bytes, and the NEXT load of the
// same wave takes the other half of each 128-byte line, so the sweep reads one state volume whatever the subset.
// Reduction, no atomics: accumulator tiles per wave over its grid-stride loop -> the waves of a workgroup added through LDS in wave
// order -> one partial row per workgroup -> launch_expect_final adds the rows in its fixed order.  Equal calls give equal bits.
//
// k_density_small (registers too small for a tile: n < 5, or fewer than four environments): one workgroup, a thread per element
// of rho, the environments added in ascending order.
#include "density.h"

namespace qsim {
namespace {

template <typename R, int KK, bool Q0IN>
__global__ __launch_bounds__(kTPB) void k_density(const R *__restrict__ amp, CtrlGeom g, uint64_t row_mask, double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int RU = density_row_units(F32, KK, Q0IN), CR = density_components(F32, Q0IN), ES = density_env_slots(F32, Q0IN);
    constexpr int NL = density_loads(RU), U = density_steps_per_trip(NL), NT = density_tiles(KK), NUT = density_upper_tiles(KK);
    constexpr int D = RU >= 16 ? 1 : 16 / RU; // lanes that share a unit
    static_assert(RU * CR == 16 * NT && (RU >= 16 ? CR * NL == NT : CR == NT * D), "every component of every unit is one operand row");
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // a scalar: so is all that follows from it
    const uint32_t i = lane & 15u, e = lane >> 4;
    [[maybe_unused]] const uint32_t d = i / (uint32_t)(RU >= 16 ? 16 : RU);

    // The lane's own part of every address of a trip, once: spread is linear over OR of disjoint bit sets, a trip starts at a
    // multiple of U steps, so index = spread(s0 << 2) [scalar] | spread(u << 2 | e) | row [this table].
    uint64_t own[U][NL];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int t = 0; t < NL; t++)
            own[u][t] = spread<R>(g, (uint64_t)(u << 2) | e) | deposit((uint32_t)(16 * t + i) & (uint32_t)(RU - 1), row_mask);

    f64x4 acc[NUT];
#pragma unroll
    for (int x = 0; x < NUT; x++) acc[x] = f64x4{0.0, 0.0, 0.0, 0.0};

    auto load_trip = [&](V(&v)[U][NL], uint64_t s0) { // a whole trip inside the register: no guard
        const uint64_t base = spread<R>(g, s0 << 2);
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int t = 0; t < NL; t++) v[u][t] = load_unit(amp, base | own[u][t]);
    };
    auto multiply = [&](const V(&v)[U][NL]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int es = 0; es < ES; es++) {
                double op[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    if constexpr (RU >= 16) op[t] = pick(v[u][t % NL], 2 * es + t / NL);
                    else if constexpr (D == 2) op[t] = (d & 1u) ? pick(v[u][0], 2 * es + t * D + 1) : pick(v[u][0], 2 * es + t * D);
                    else {
                        // One of four: selects on VALUES by the bits of d.  The empty asm hides from the compiler that the candidates
                        // are components of one unit — it turns plain selects into a lane-indexed read of the unit through scratch
                        // memory, which at n = 30 took 6.9 ms where this takes 2.7.  (One of two, above: the asm gained nothing,
                        // 4.2 ms against 4.5; what these shapes' time depends on is not understood yet)
                        double p[D];
#pragma unroll
                        for (int dd = 0; dd < D; dd++) {
                            p[dd] = pick(v[u][0], 2 * es + t * D + dd);
                            asm("" : "+v"(p[dd]));
                        }
                        op[t] = (d & 2u) ? ((d & 1u) ? p[3] : p[2]) : ((d & 1u) ? p[1] : p[0]);
                    }
                }
                int x = 0;
#pragma unroll
                for (int s = 0; s < NT; s++)
#pragma unroll
                    for (int t = s; t < NT; t++, x++) acc[x] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[s], op[t], acc[x], 0, 0, 0);
            }
        }
    };

    const uint64_t steps = (g.units + 3ULL) >> 2; // four environment units per step
    const uint64_t first = ((uint64_t)blockIdx.x * kDensityWaves + wave) * U, stride = (uint64_t)gridDim.x * kDensityWaves * U;
    if (g.units < 4ULL * U) {
        // fewer environment units than one trip has (a power of two below 4 U): one guarded trip of one wave
        if (first == 0) {
            V v[U][NL];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int t = 0; t < NL; t++) {
                    v[u][t] = V{};
                    if (((uint64_t)(u << 2) | e) < g.units) v[u][t] = load_unit(amp, own[u][t]);
                }
            multiply(v);
        }
    } else {
        // every trip is whole: steps is a multiple of U.  All loads of a trip first, then its products; the other waves of the SIMD
        // cover the wait (a second register set for the next trip's loads doubled the accumulators the compiler kept: not built).
        for (uint64_t s0 = first; s0 < steps; s0 += stride) {
            V v[U][NL];
            load_trip(v, s0);
            multiply(v);
        }
    }

    // the waves of the workgroup, in wave order, into wave 0
    __shared__ double red[NUT * 256];
    for (uint32_t w = 1; w < (uint32_t)kDensityWaves; w++) {
        if (wave == w) {
#pragma unroll
            for (int x = 0; x < NUT; x++)
#pragma unroll
                for (int r = 0; r < 4; r++) red[(x * 4 + r) * 64 + lane] = acc[x][r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int x = 0; x < NUT; x++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[x][r] += red[(x * 4 + r) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave == 0) {
        double *out = partial + (size_t)blockIdx.x * (NUT * 256);
#pragma unroll
        for (int x = 0; x < NUT; x++)
#pragma unroll
            for (int r = 0; r < 4; r++) out[(x * 4 + r) * 64 + lane] = acc[x][r];
    }
}

// out[(a * 2^k + a') * 2 + (0, 1)] = (Re, Im) sum_b psi(a, b) conj(psi(a', b)), a and a' over the sorted subset `mask`
template <typename R>
__global__ __launch_bounds__(kTPB) void k_density_small(const R *__restrict__ amp, uint64_t mask, uint64_t env_mask, int k, int env_bits,
                                                        double *__restrict__ out) {
    const uint32_t dim = 1u << k, envs = 1u << env_bits;
    for (uint32_t el = threadIdx.x; el < dim * dim; el += kTPB) {
        const uint64_t ja = deposit(el >> k, mask), jb = deposit(el & (dim - 1u), mask);
        double re = 0.0, im = 0.0;
        for (uint32_t b = 0; b < envs; b++) {
            const uint64_t jenv = deposit(b, env_mask);
            const double pr = (double)amp[2 * (ja | jenv)], pi = (double)amp[2 * (ja | jenv) + 1];
            const double qr = (double)amp[2 * (jb | jenv)], qi = (double)amp[2 * (jb | jenv) + 1];
            re += fma(pr, qr, pi * qi);
            im += fma(pi, qr, -(pr * qi));
        }
        out[2 * el] = re;
        out[2 * el + 1] = im;
    }
}

template <typename R, int KK, bool Q0IN>
hipError_t launch_shape(hipStream_t stream, const void *amps, const DensityPlan &p, double *d_scratch) {
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int U = density_steps_per_trip(density_loads(density_row_units(F32, KK, Q0IN)));
    const CtrlGeom g = ctrl_geom(p.mask, 0, F32, p.n); // units: the environment units; zeros: where the subset's bits go
    if (g.units != p.env_units) return hipErrorInvalidValue;
    const uint64_t row_mask = p.mask & ~(uint64_t)(F32 ? 1 : 0); // fp32: index bit 0 is the slot, inside the unit
    const unsigned grid = reducing_grid<k_density<R, KK, Q0IN>>((g.units + 3ULL) >> 2, (uint64_t)kDensityWaves * U);
    hipLaunchKernelGGL((k_density<R, KK, Q0IN>), dim3(grid), dim3(kTPB), 0, stream, (const R *)amps, g, row_mask, d_scratch);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_expect_final(stream, d_scratch, (int)grid, density_row_doubles(KK), density_result(p, d_scratch));
}

template <typename R, bool Q0IN>
hipError_t launch_prec(hipStream_t stream, const void *amps, const DensityPlan &p, double *d_scratch) {
    return for_subset_size(p.padded_k, [&](auto kk) { return launch_shape<R, decltype(kk)::value, Q0IN>(stream, amps, p, d_scratch); });
}

} // namespace

size_t density_scratch_doubles(const DensityPlan &p) {
    if (!p.path) return (size_t)2 << (2 * p.k);
    return ((size_t)kExpectGrid + 1) * density_row_doubles(p.padded_k);
}

hipError_t launch_density(const LaunchCfg &cfg, const void *amps, const DensityPlan &p, double *d_scratch) {
    if (!amps || !d_scratch || p.n < 0 || p.n > 40 || (p.mask & ~index_mask(p.n))) return hipErrorInvalidValue;
    if (!p.path) {
        if (p.k != __builtin_popcountll(p.mask) || p.n - p.k > 8) return hipErrorInvalidValue;
        const uint64_t env_mask = index_mask(p.n) & ~p.mask;
        if (p.f32) hipLaunchKernelGGL(k_density_small<float>, dim3(1), dim3(kTPB), 0, cfg.stream, (const float *)amps, p.mask, env_mask, p.k, p.n - p.k, d_scratch);
        else hipLaunchKernelGGL(k_density_small<double>, dim3(1), dim3(kTPB), 0, cfg.stream, (const double *)amps, p.mask, env_mask, p.k, p.n - p.k, d_scratch);
        return hipGetLastError();
    }
    if (p.padded_k != __builtin_popcountll(p.mask) || p.n - p.padded_k < 2 || p.q0_in != (bool)(p.mask & 1ULL)) return hipErrorInvalidValue;
    if (!p.f32) return launch_prec<double, false>(cfg.stream, amps, p, d_scratch); // fp64: a unit is one amplitude wherever qubit 0 is
    return p.q0_in ? launch_prec<float, true>(cfg.stream, amps, p, d_scratch) : launch_prec<float, false>(cfg.stream, amps, p, d_scratch);
}

} // namespace qsim
