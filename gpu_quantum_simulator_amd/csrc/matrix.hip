// matrix.hip — a dense matrix on up to five target qubits, under any number of controls, as ONE in-place sweep of the control
// subspace on the matrix cores (gfx950).  Its own object, like density.hip, whose walk it shares: nothing here is compiled into
// kernels.hip.  matrix.h has the decomposition (R' = M R in 16 x 16 tiles, which rows a lane owns, the shapes), subset_sweep.h what
// density.hip uses too, and matrix.cpp the host side; this file has the two kernels.
//
// k_matrix (the matrix path).  A wave works on its own.  Lane l = (e = l & 15, g = l >> 4) loads the units of environment unit
// 16 step + e whose unit-row index is g (mod 4), all of a trip first; a component of such a unit IS the lane's element
// B[l >> 4][l & 15] of a 4 x 16 slice of R, and the lane's coefficient registers are its elements A[l & 15][l >> 4] of the 16 x 4
// slices of M, so result tile t is the chain acc[t] = mfma(m[t][s], r[s], acc[t]) over the slices s — and by the D map (col = l & 15,
// row = (l >> 4) + 4 reg) the lane receives exactly the rows it supplied.  It stores them to the addresses it loaded: no LDS, no
// shuffle, no barrier (a wave has loaded all rows of its environments before any of its results exists, and environments are
// disjoint between waves).  Every stored amplitude comes from one wave in one fixed order: equal calls give equal bits whatever
// the grid is.  fp32 components are widened and the products are fp64: one kernel body and one row order of M for both
// precisions, and an fp32 result is the fp64 one rounded once; the f32 matrix instruction is not built.
// Addresses as in density.hip: spread(CtrlGeom) with zeros = subset and controls, ones = the controls; the step's part is
// wave-uniform (scalar unit), the lane's part is a table formed once.
//
// k_matrix_small (fewer than 16 environment units): one workgroup, a thread per amplitude of the control subspace (at most
// kMatrixSmallPerThread each), all sums formed before the barrier, all stores behind it; the caller's U and order, nothing padded.
#include "matrix.h"

namespace qsim {
namespace {

template <typename R, int KK, int MODE>
__global__ __launch_bounds__(kTPB) void k_matrix(R *amp, CtrlGeom g, uint64_t row_mask, const double *__restrict__ coef) {
    using V = typename Vec16<R>::type;
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int S = matrix_slices(KK), T = matrix_tiles(KK), CR = matrix_components(F32, MODE);
    constexpr int NU = matrix_lane_units(F32, KK, MODE), U = matrix_steps_per_trip(NU);
    // rounds of products per load: the slots of an fp32 unit that are environments of their own (a control on qubit 0: the odd one alone)
    constexpr int E0 = F32 && MODE == kMatrixCtrl ? 1 : 0, E1 = F32 && MODE != kMatrixRows ? 2 : 1;
    static_assert(NU * CR == S && S == 4 * T && (U & (U - 1)) == 0, "a lane's units are its S real rows; a trip starts at a multiple of U steps");
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // a scalar: so is all that follows from it
    const uint32_t e = lane & 15u, gg = lane >> 4;

    double m[T][S]; // the lane's elements of the A operands: 4, 16 or 64 registers
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int s = 0; s < S; s++) m[t][s] = coef[(size_t)(t * S + s) * 64 + lane];

    // The lane's own part of every address of a trip, once: spread is linear over OR of disjoint bit sets and a trip starts at a
    // multiple of U steps, so index = spread(s0 << 4) [scalar] | spread(u << 4 | e) | controls | unit row [this table].
    uint64_t own[U][NU];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int q = 0; q < NU; q++) own[u][q] = spread<R>(g, (uint64_t)(u << 4) | e) | g.ones | deposit(gg + 4u * (uint32_t)q, row_mask);

    // one step: the products of its 16 environment units (per round) and the stores
    auto step = [&](const V(&v)[NU], uint64_t at0, const uint64_t(&at)[NU]) {
        R res[2][S];
#pragma unroll
        for (int es = E0; es < E1; es++) {
            f64x4 acc[T];
#pragma unroll
            for (int t = 0; t < T; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < S; s++) {
                const double r = pick(v[s / CR], (F32 && MODE != kMatrixRows ? 2 * es : 0) + s % CR);
#pragma unroll
                for (int t = 0; t < T; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[t][s], r, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < S; j++) res[es][j] = (R)acc[j >> 2][j & 3];
        }
#pragma unroll
        for (int q = 0; q < NU; q++) {
            V out;
            if constexpr (!F32) out = V{res[0][2 * q], res[0][2 * q + 1]};
            else if constexpr (MODE == kMatrixRows) out = V{res[0][4 * q], res[0][4 * q + 1], res[0][4 * q + 2], res[0][4 * q + 3]};
            else if constexpr (MODE == kMatrixEnvs) out = V{res[0][2 * q], res[0][2 * q + 1], res[1][2 * q], res[1][2 * q + 1]};
            else out = V{v[q].x, v[q].y, res[1][2 * q], res[1][2 * q + 1]}; // the even slot lies outside the control subspace: as loaded
            *reinterpret_cast<V *>(amp + 2 * (at0 | at[q])) = out;
        }
    };

    const uint64_t steps = g.units >> 4; // 16 environment units per step; units is a power of two, at least 16
    const uint64_t first = ((uint64_t)blockIdx.x * kMatrixWaves + wave) * U, stride = (uint64_t)gridDim.x * kMatrixWaves * U;
    if (steps < (uint64_t)U) {
        // fewer steps than one trip has (a power of two below U): one guarded trip of one wave; the guard is wave-uniform
        if (first == 0) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                if ((uint64_t)u >= steps) break;
                V v[NU];
#pragma unroll
                for (int q = 0; q < NU; q++) v[q] = load_unit(amp, own[u][q]);
                step(v, 0, own[u]);
            }
        }
        return;
    }
    // every trip is whole: steps is a multiple of U.  All loads of a trip first, then step by step its products and its stores.
    for (uint64_t s0 = first; s0 < steps; s0 += stride) {
        const uint64_t base = spread<R>(g, s0 << 4);
        V v[U][NU];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int q = 0; q < NU; q++) v[u][q] = load_unit(amp, base | own[u][q]);
#pragma unroll
        for (int u = 0; u < U; u++) step(v[u], base, own[u]);
    }
}

struct SmallArgs { // by value: a kernel argument
    uint64_t env_mask, ones; // the index bits that are neither targets nor controls; the controls
    int32_t k, env_bits;
    int32_t target[kMatrixMaxQubits]; // bit j of a row or column index of U is index bit target[j]
};

__device__ __forceinline__ uint64_t target_index(const SmallArgs &a, uint32_t r) {
    uint64_t j = 0;
    for (int b = 0; b < a.k; b++) j |= (uint64_t)((r >> b) & 1u) << a.target[b];
    return j;
}

// amp[base(b) | T(r)] <- sum_c U[r][c] amp[base(b) | T(c)] for every environment b of the control subspace, fp64 sums
template <typename R>
__global__ __launch_bounds__(kTPB) void k_matrix_small(R *amp, SmallArgs a, const double *__restrict__ U) {
    const uint32_t dim = 1u << a.k, outs = dim << a.env_bits;
    double yr[kMatrixSmallPerThread], yi[kMatrixSmallPerThread];
#pragma unroll
    for (int p = 0; p < kMatrixSmallPerThread; p++) {
        const uint32_t o = threadIdx.x + (uint32_t)p * kTPB;
        yr[p] = yi[p] = 0.0;
        if (o >= outs) continue;
        const uint32_t r = o & (dim - 1u);
        const uint64_t base = deposit(o >> a.k, a.env_mask) | a.ones;
        for (uint32_t c = 0; c < dim; c++) {
            const uint64_t j = base | target_index(a, c);
            const double xr = (double)amp[2 * j], xi = (double)amp[2 * j + 1];
            const double ur = U[2 * (r * dim + c)], ui = U[2 * (r * dim + c) + 1];
            yr[p] = fma(ur, xr, fma(-ui, xi, yr[p]));
            yi[p] = fma(ur, xi, fma(ui, xr, yi[p]));
        }
    }
    __syncthreads(); // in place: every sum is formed before any amplitude is replaced
#pragma unroll
    for (int p = 0; p < kMatrixSmallPerThread; p++) {
        const uint32_t o = threadIdx.x + (uint32_t)p * kTPB;
        if (o >= outs) continue;
        const uint64_t j = deposit(o >> a.k, a.env_mask) | a.ones | target_index(a, o & (dim - 1u));
        amp[2 * j] = (R)yr[p];
        amp[2 * j + 1] = (R)yi[p];
    }
}

template <typename R, int KK, int MODE>
hipError_t launch_shape(const LaunchCfg &cfg, void *amps, const MatrixPlan &p, const double *d_coef) {
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int NU = matrix_lane_units(F32, KK, MODE), U = matrix_steps_per_trip(NU);
    const CtrlGeom g = matrix_geom(p.mask, p.controls, F32, p.n);
    const uint64_t row_mask = p.mask & ~(uint64_t)(F32 ? 1 : 0); // fp32: index bit 0 is the slot, inside the unit
    // every address is spread(environment unit) | controls | deposit(unit row): inside the buffer when the three bit sets are what
    // the kernel's shape takes them for
    if (g.units != p.env_units || g.units < (uint64_t)kMatrixEnvsPerStep || (g.units & (g.units - 1ULL)) != 0) return hipErrorInvalidValue;
    if ((1 << __builtin_popcountll(row_mask)) != 4 * NU) return hipErrorInvalidValue;
    if ((g.units << __builtin_popcountll(g.zeros)) != (1ULL << p.n) >> (F32 ? 1 : 0)) return hipErrorInvalidValue;
    unsigned grid = writing_grid<k_matrix<R, KK, MODE>>(cfg, g.units >> 4, (uint64_t)kMatrixWaves * U);
    if (cfg.grid_cap <= 0 && grid > (unsigned)matrix_grid_cap(KK)) grid = (unsigned)matrix_grid_cap(KK);
    hipLaunchKernelGGL((k_matrix<R, KK, MODE>), dim3(grid), dim3(kTPB), 0, cfg.stream, (R *)amps, g, row_mask, d_coef);
    return hipGetLastError();
}

template <typename R, int MODE>
hipError_t launch_prec(const LaunchCfg &cfg, void *amps, const MatrixPlan &p, const double *d_coef) {
    return for_subset_size(p.padded_k, [&](auto kk) { return launch_shape<R, decltype(kk)::value, MODE>(cfg, amps, p, d_coef); });
}

} // namespace

hipError_t launch_matrix(const LaunchCfg &cfg, void *amps, const MatrixPlan &p, const double *d_coef) {
    const uint64_t all = index_mask(p.n);
    if (!amps || !d_coef || p.n < 0 || p.n > 40 || ((p.mask | p.controls) & ~all) || (p.mask & p.controls)) return hipErrorInvalidValue;
    if (p.num_controls != __builtin_popcountll(p.controls)) return hipErrorInvalidValue;
    if (!p.path) {
        const int env_bits = p.n - p.k - p.num_controls;
        if (p.k != __builtin_popcountll(p.mask) || p.k > kMatrixMaxQubits || env_bits < 0 || ((uint64_t)1 << (p.k + env_bits)) > (uint64_t)kTPB * kMatrixSmallPerThread)
            return hipErrorInvalidValue;
        SmallArgs a{};
        a.env_mask = all & ~(p.mask | p.controls), a.ones = p.controls, a.k = p.k, a.env_bits = env_bits;
        uint64_t seen = 0;
        for (int j = 0; j < p.k; j++) {
            if (p.targets[j] < 0 || p.targets[j] >= p.n) return hipErrorInvalidValue;
            a.target[j] = p.targets[j], seen |= 1ULL << p.targets[j];
        }
        if (seen != p.mask) return hipErrorInvalidValue;
        if (p.f32) hipLaunchKernelGGL(k_matrix_small<float>, dim3(1), dim3(kTPB), 0, cfg.stream, (float *)amps, a, d_coef);
        else hipLaunchKernelGGL(k_matrix_small<double>, dim3(1), dim3(kTPB), 0, cfg.stream, (double *)amps, a, d_coef);
        return hipGetLastError();
    }
    if (p.padded_k != __builtin_popcountll(p.mask)) return hipErrorInvalidValue;
    const int mode = !p.f32 || (p.mask & 1ULL) ? kMatrixRows : (p.controls & 1ULL) ? kMatrixCtrl : kMatrixEnvs;
    if (mode != p.mode) return hipErrorInvalidValue;
    if (!p.f32) return launch_prec<double, kMatrixRows>(cfg, amps, p, d_coef);
    switch (mode) {
    case kMatrixRows: return launch_prec<float, kMatrixRows>(cfg, amps, p, d_coef);
    case kMatrixEnvs: return launch_prec<float, kMatrixEnvs>(cfg, amps, p, d_coef);
    default: return launch_prec<float, kMatrixCtrl>(cfg, amps, p, d_coef);
    }
}

} // namespace qsim
