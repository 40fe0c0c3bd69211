// subsystem.hip — reduced density matrices of 6 to 10 qubits: G = R R^T in blocks of 128 rows and slices of the environments, on
// the matrix cores (gfx950).  Its own object, like density.hip.  subsystem.h has the decomposition (the interleaved rows of R, blocks,
// chunks, slices) and subsystem.cpp the host side; this file has the kernels.
//
// k_subsystem (path 1), instantiated for the blocks off the diagonal and for the diagonal ones and launched in that order.  One
// workgroup per (block, slice), the block index fastest, so the workgroups that run together share their panels in the caches.  Per chunk of E = 32 environments the workgroup stages the panel of block row bi
// (64 rows of Psi x E environments = 128 rows of R, widened to fp64) and, off the diagonal, the panel of bj in LDS: thread tid loads
// the units t = tid + 256 it of the panel, t counting through the index bits that are free inside a (block, chunk) — the six lowest
// subset bits and the five lowest environment bits — lowest first, so consecutive lanes take consecutive units and every
// 128-byte line of a panel is read whole, wherever the subset lies.  fp32: a unit is two amplitudes and index bit 0 is never among
// the free bits; its second amplitude is the next row of Psi (qubit 0 in the subset) or the next environment (outside).  The
// address is (chunk's environment bits | block's row bits) [scalar] | the thread's own table, computed once.  A panel lies in LDS as
// [environment][row of R] with a stride of 144 doubles: lane l of a wave reads (row i = l & 15, environment l >> 4) — which IS the
// operand element of v_mfma_f64_16x16x4_f64 for A and for B — with one ds_read_b64, free of bank conflicts.  Wave w multiplies
// the quarter (rows 64 (w >> 1), columns 64 (w & 1)): four A and four B operands per step of four environments, 16 products; in a
// diagonal block, which is symmetric and has one panel, nine of the 36 tiles with row <= column (diag_products).  The
// next chunk's units are loaded into registers before the products of this one.  Every sum is fp64; fp32 products are exact.
// The block is written row-major to partial (slice, block).
// k_subsystem_final: result[block][el] = the S partials added in ascending slice order, one thread per element.
// k_subsystem_plain (path 0: one or two environments): a thread per element of rho over a grid-stride loop.
#include "subsystem.h"

namespace qsim {
namespace {

struct SubGeom {          // by value: a kernel argument
    uint64_t sub_mask;    // the subset
    uint64_t env_mask;    // every other index bit of the register
    uint64_t free_mask;   // the index bits a thread's t counts through (fp32: without bit 0)
    uint64_t row_low;     // the six lowest subset bits
    uint64_t env_low;     // the chunk_env_bits lowest environment bits
    uint32_t units;       // 16-byte units of one panel and chunk
    uint32_t env_bits;    // log2 environments per chunk (2..5)
    uint32_t blocks, upper_blocks;
    uint64_t trips;       // chunks per slice
    uint32_t slot1;       // fp32: doubles from a unit's first amplitude to its second in a panel
};

__device__ __forceinline__ uint64_t deposit64(uint64_t v, uint64_t mask) { // bit j of v -> the j-th lowest set bit of mask
    uint64_t r = 0;
    for (uint64_t m = mask; m != 0; m &= m - 1ULL, v >>= 1)
        if (v & 1ULL) r |= m & (0ULL - m);
    return r;
}
__device__ __forceinline__ uint32_t extract64(uint64_t idx, uint64_t mask) { // the inverse: the j-th lowest set bit of mask -> bit j
    uint32_t r = 0, j = 0;
    for (uint64_t m = mask; m != 0; m &= m - 1ULL, j++)
        if (idx & m & (0ULL - m)) r |= 1u << j;
    return r;
}

// A diagonal block is symmetric: of its 8 x 8 tiles only the 36 with row <= column are multiplied, nine per wave — wave w takes tile
// rows w (columns w..7) and 7 - w (columns 7 - w..7).  acc[i], i < 8 - w: tile (w, w + i); the others: tile (7 - w, i - 1).  One
// instruction stream for the four waves: w, a scalar, enters addresses and selects on values only.  (A loop per w, or products
// under uniform branches, made the compiler copy accumulator tuples and cost the kernel half its occupancy.)  A and B operands of
// one panel have the same lane map, so both are read through pl.
__device__ __forceinline__ uint32_t diag_row(uint32_t w, int i) { return (uint32_t)i < 8u - w ? w : 7u - w; }
__device__ __forceinline__ uint32_t diag_col(uint32_t w, int i) { return (uint32_t)i < 8u - w ? w + (uint32_t)i : (uint32_t)i - 1u; }
__device__ __forceinline__ void diag_products(f64x4 (&acc)[16], const double *pl, uint32_t steps, uint32_t w) {
    for (uint32_t st = 0; st < steps; st++) {
        const double *p = pl + st * 4 * kSubPanelStride;
        const double a0 = p[16 * w], a1 = p[16 * (7 - w)];
        double b[9];
#pragma unroll
        for (int i = 0; i < 9; i++) b[i] = p[16 * diag_col(w, i)];
#pragma unroll
        for (int i = 0; i < 9; i++) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64((uint32_t)i < 8u - w ? a0 : a1, b[i], acc[i], 0, 0, 0);
    }
}
// C/D: col = lane & 15, row = (lane >> 4) + 4 reg.  The tiles below the diagonal, which nobody multiplies, are written as zeros.
__device__ __forceinline__ void diag_store(const f64x4 (&acc)[16], double *out, uint32_t lane, uint32_t w) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const uint32_t row = diag_row(w, i), col = diag_col(w, i);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            out[(size_t)(16 * row + (lane >> 4) + 4 * r) * kSubBlockRows + 16 * col + (lane & 15u)] = acc[i][r];
            if (col != row) out[(size_t)(16 * col + (lane >> 4) + 4 * r) * kSubBlockRows + 16 * row + (lane & 15u)] = 0.0;
        }
    }
}

template <typename R, bool DIAG>
__global__ __launch_bounds__(kTPB) void k_subsystem(const R *__restrict__ amp, SubGeom g, double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int IT = ((1 << (kSubBlockAmpBits + kSubChunkEnvBits)) >> (F32 ? 1 : 0)) / kTPB; // units of a panel per thread: 8, 4
    __shared__ __attribute__((aligned(16))) double lds[(DIAG ? 1 : 2) * kSubPanelDoubles];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // which block and slice: the diagonal blocks in order, or the blocks bi < bj row by row
    constexpr bool diag = DIAG;
    const uint32_t per_slice = DIAG ? g.blocks : g.upper_blocks - g.blocks;
    const uint32_t slice = blockIdx.x / per_slice;
    uint32_t bj = blockIdx.x - slice * per_slice, bi = DIAG ? bj : 0;
    if constexpr (!DIAG) {
        while (bj >= g.blocks - 1 - bi) bj -= g.blocks - 1 - bi, bi++;
        bj += bi + 1;
    }
    const uint32_t block = bi * g.blocks - bi * (bi - 1) / 2 + (bj - bi); // subsystem_block_index
    const uint64_t rows_i = deposit64((uint64_t)bi << kSubBlockAmpBits, g.sub_mask), rows_j = deposit64((uint64_t)bj << kSubBlockAmpBits, g.sub_mask);

    // the thread's own units: where they lie in the state and in a panel
    uint64_t own[IT];
    uint32_t at[IT];
#pragma unroll
    for (int it = 0; it < IT; it++) {
        own[it] = deposit64((uint64_t)(it * kTPB) + tid, g.free_mask);
        at[it] = extract64(own[it], g.env_low) * (uint32_t)kSubPanelStride + 2u * extract64(own[it], g.row_low);
    }

    V va[IT] = {}, vb[IT] = {};
    auto fetch = [&](uint64_t chunk) {
        const uint64_t env = deposit64(chunk << g.env_bits, g.env_mask);
#pragma unroll
        for (int it = 0; it < IT; it++) {
            if ((uint32_t)(it * kTPB) + tid < g.units) {
                va[it] = load_unit(amp, env | rows_i | own[it]);
                if (!diag) vb[it] = load_unit(amp, env | rows_j | own[it]);
            }
        }
    };
    auto put = [&](double *panel, const V(&v)[IT]) {
#pragma unroll
        for (int it = 0; it < IT; it++)
            if ((uint32_t)(it * kTPB) + tid < g.units) {
                if constexpr (F32) {
                    *reinterpret_cast<double2 *>(panel + at[it]) = double2{(double)v[it].x, (double)v[it].y};
                    *reinterpret_cast<double2 *>(panel + at[it] + g.slot1) = double2{(double)v[it].z, (double)v[it].w};
                } else *reinterpret_cast<double2 *>(panel + at[it]) = v[it];
            }
    };

    f64x4 acc[16]; // off the diagonal: acc[4 s + t] is tile (s, t) of the wave's quarter
#pragma unroll
    for (int x = 0; x < 16; x++) acc[x] = f64x4{0.0, 0.0, 0.0, 0.0};
    const uint32_t rq = (wave >> 1) * 64u, cq = (wave & 1u) * 64u;
    const double *pl = lds + (lane >> 4) * kSubPanelStride + (lane & 15u);
    const double *pa = pl + rq, *pb = pl + kSubPanelDoubles + cq;
    const uint32_t steps = (1u << g.env_bits) >> 2;

    const uint64_t first = (uint64_t)slice * g.trips;
    fetch(first);
    for (uint64_t trip = 0; trip < g.trips; trip++) {
        __syncthreads(); // the products of the chunk before are done with the panels
        put(lds, va);
        if (!diag) put(lds + kSubPanelDoubles, vb);
        __syncthreads();
        if (trip + 1 < g.trips) fetch(first + trip + 1);
        if constexpr (DIAG) diag_products(acc, pl, steps, wave);
        else {
            for (uint32_t st = 0; st < steps; st++) {
                double a[4], b[4];
#pragma unroll
                for (int s = 0; s < 4; s++) a[s] = pa[st * 4 * kSubPanelStride + 16 * s], b[s] = pb[st * 4 * kSubPanelStride + 16 * s];
#pragma unroll
                for (int s = 0; s < 4; s++)
#pragma unroll
                    for (int t = 0; t < 4; t++) acc[4 * s + t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[t], acc[4 * s + t], 0, 0, 0);
            }
        }
    }

    double *out = partial + ((size_t)slice * g.upper_blocks + block) * kSubBlockDoubles;
    if constexpr (DIAG) {
        diag_store(acc, out, lane, wave);
        return;
    }
    // C/D: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) out[(size_t)(rq + 16 * s + (lane >> 4) + 4 * r) * kSubBlockRows + cq + 16 * t + (lane & 15u)] = acc[4 * s + t][r];
}

__global__ __launch_bounds__(kTPB) void k_subsystem_final(const double *__restrict__ partial, uint64_t count, uint32_t slices, double *__restrict__ out) {
    for (uint64_t el = (uint64_t)blockIdx.x * kTPB + threadIdx.x; el < count; el += (uint64_t)gridDim.x * kTPB) {
        double sum = partial[el];
        for (uint32_t s = 1; s < slices; s++) sum += partial[(uint64_t)s * count + el];
        out[el] = sum;
    }
}

// out[(a * 2^k + a') * 2 + (0, 1)] = (Re, Im) sum_b psi(a, b) conj(psi(a', b)), a and a' over the sorted subset `mask`
template <typename R>
__global__ __launch_bounds__(kTPB) void k_subsystem_plain(const R *__restrict__ amp, uint64_t mask, uint64_t env_mask, int k, int env_bits,
                                                          double *__restrict__ out) {
    const uint64_t dim = 1ULL << k, envs = 1ULL << env_bits;
    for (uint64_t el = (uint64_t)blockIdx.x * kTPB + threadIdx.x; el < dim * dim; el += (uint64_t)gridDim.x * kTPB) {
        const uint64_t ja = deposit64(el >> k, mask), jb = deposit64(el & (dim - 1ULL), mask);
        double re = 0.0, im = 0.0;
        for (uint64_t b = 0; b < envs; b++) {
            const uint64_t jenv = deposit64(b, env_mask);
            const double pr = (double)amp[2 * (ja | jenv)], pi = (double)amp[2 * (ja | jenv) + 1];
            const double qr = (double)amp[2 * (jb | jenv)], qi = (double)amp[2 * (jb | jenv) + 1];
            re += fma(pr, qr, pi * qi);
            im += fma(pi, qr, -(pr * qi));
        }
        out[2 * el] = re;
        out[2 * el + 1] = im;
    }
}

// the arithmetic yardstick: the sweep's 16 accumulator tiles and nothing else.  The accumulators leave through stores, as the
// sweep's do (summed in vector code they were copied between the register files every round), and only where out_stride says so.
__global__ __launch_bounds__(kTPB) void k_mfma_probe(long rounds, size_t out_stride, double *__restrict__ out) {
    extern __shared__ double unused[];
    f64x4 acc[16];
#pragma unroll
    for (int x = 0; x < 16; x++) acc[x] = f64x4{0.0, 0.0, 0.0, 0.0};
    double a[4], b[4];
#pragma unroll
    for (int s = 0; s < 4; s++) a[s] = 1.0 + (double)(threadIdx.x + s) * 0x1p-20, b[s] = 1.0 - (double)(threadIdx.x + 2 * s) * 0x1p-20;
    for (long r = 0; r < rounds; r += 8)
        for (int st = 0; st < 8; st++) {
#pragma unroll
            for (int s = 0; s < 4; s++) asm volatile("" : "+v"(a[s]), "+v"(b[s])); // operands of this step, as far as the compiler knows
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int t = 0; t < 4; t++) acc[4 * s + t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[t], acc[4 * s + t], 0, 0, 0);
        }
    if (out_stride == 0 && blockIdx.x != 0) return; // one workgroup's worth of results is enough to keep the products
    double *o = out + (size_t)blockIdx.x * out_stride + threadIdx.x;
#pragma unroll
    for (int x = 0; x < 16; x++)
#pragma unroll
        for (int r = 0; r < 4; r++) o[(size_t)(4 * x + r) * kTPB] = acc[x][r];
}

uint64_t lowest_bits(uint64_t mask, int count) {
    uint64_t r = 0;
    for (; mask != 0 && count > 0; mask &= mask - 1ULL, count--) r |= mask & (0ULL - mask);
    return r;
}

} // namespace

hipError_t launch_subsystem(hipStream_t stream, const void *amps, const SubsystemPlan &p, double *d_scratch) {
    if (!amps || !d_scratch || p.n < 0 || p.n > 40 || (p.mask & ~index_mask(p.n)) || p.k != __builtin_popcountll(p.mask)) return hipErrorInvalidValue;
    const uint64_t env_mask = index_mask(p.n) & ~p.mask;
    if (!p.path) {
        if (p.n - p.k > 1 || p.k > kSubsystemMaxQubits) return hipErrorInvalidValue;
        const uint64_t elements = 1ULL << (2 * p.k);
        const unsigned grid = (unsigned)std::min<uint64_t>((elements + kTPB - 1) / kTPB, kSubPlainGrid);
        if (p.f32) hipLaunchKernelGGL(k_subsystem_plain<float>, dim3(grid), dim3(kTPB), 0, stream, (const float *)amps, p.mask, env_mask, p.k, p.n - p.k, d_scratch);
        else hipLaunchKernelGGL(k_subsystem_plain<double>, dim3(grid), dim3(kTPB), 0, stream, (const double *)amps, p.mask, env_mask, p.k, p.n - p.k, d_scratch);
        return hipGetLastError();
    }
    if (p.k < kSubsystemMinQubits || p.k > kSubsystemMaxQubits || p.n - p.k < 2 || p.block_rows != kSubBlockRows || p.blocks != (2L << p.k) / kSubBlockRows ||
        p.upper_blocks != p.blocks * (p.blocks + 1) / 2 || p.chunk_env_bits < 2 || p.chunk_env_bits > kSubChunkEnvBits || p.slices < 1 || p.trips < 1 ||
        (uint64_t)p.slices * p.trips << p.chunk_env_bits != 1ULL << (p.n - p.k) || p.slices * p.upper_blocks > kSubMaxPartialBlocks)
        return hipErrorInvalidValue;
    SubGeom g{};
    g.sub_mask = p.mask, g.env_mask = env_mask;
    g.row_low = lowest_bits(p.mask, kSubBlockAmpBits), g.env_low = lowest_bits(env_mask, p.chunk_env_bits);
    g.free_mask = (g.row_low | g.env_low) & ~(uint64_t)(p.f32 ? 1 : 0);
    g.units = (uint32_t)((1u << (kSubBlockAmpBits + p.chunk_env_bits)) >> (p.f32 ? 1 : 0));
    g.env_bits = p.chunk_env_bits;
    g.blocks = (uint32_t)p.blocks, g.upper_blocks = (uint32_t)p.upper_blocks;
    g.trips = (uint64_t)p.trips;
    g.slot1 = p.mask & 1ULL ? 2u : (uint32_t)kSubPanelStride; // the next row of Psi, or the next environment
    const unsigned off = (unsigned)(p.slices * (p.upper_blocks - p.blocks)), on = (unsigned)(p.slices * p.blocks);
    hipError_t e = hipSuccess;
    if (off > 0) { // the blocks off the diagonal first: they are the many
        if (p.f32) hipLaunchKernelGGL((k_subsystem<float, false>), dim3(off), dim3(kTPB), 0, stream, (const float *)amps, g, d_scratch);
        else hipLaunchKernelGGL((k_subsystem<double, false>), dim3(off), dim3(kTPB), 0, stream, (const double *)amps, g, d_scratch);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (p.f32) hipLaunchKernelGGL((k_subsystem<float, true>), dim3(on), dim3(kTPB), 0, stream, (const float *)amps, g, d_scratch);
    else hipLaunchKernelGGL((k_subsystem<double, true>), dim3(on), dim3(kTPB), 0, stream, (const double *)amps, g, d_scratch);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint64_t count = (uint64_t)p.upper_blocks * kSubBlockDoubles;
    hipLaunchKernelGGL(k_subsystem_final, dim3((unsigned)std::min<uint64_t>(count / kTPB, 4096)), dim3(kTPB), 0, stream, d_scratch, count, (uint32_t)p.slices,
                       subsystem_result(p, d_scratch));
    return hipGetLastError();
}

hipError_t launch_mfma_probe(long instructions, int workgroups, int lds_bytes, float *ms) {
    if (instructions < 16 || workgroups < 1 || workgroups > 65536 || lds_bytes < 0 || lds_bytes > 160 * 1024 || !ms) return hipErrorInvalidValue;
    double *d_out = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t e = hipMalloc((void **)&d_out, (size_t)64 * kTPB * sizeof(double));
    if (e != hipSuccess) return e;
    if ((e = hipEventCreate(&ev[0])) == hipSuccess && (e = hipEventCreate(&ev[1])) == hipSuccess) {
        if (lds_bytes > 64 * 1024) e = hipFuncSetAttribute((const void *)k_mfma_probe, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        for (int run = 0; run < 2 && e == hipSuccess; run++) { // the first run warms
            (void)hipEventRecord(ev[0], nullptr);
            hipLaunchKernelGGL(k_mfma_probe, dim3(workgroups), dim3(kTPB), (size_t)lds_bytes, nullptr, instructions / 16, (size_t)0, d_out);
            e = hipGetLastError();
            (void)hipEventRecord(ev[1], nullptr);
            if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
        }
        if (e == hipSuccess) e = hipEventElapsedTime(ms, ev[0], ev[1]);
    }
    if (ev[0]) (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    (void)hipFree(d_out);
    return e;
}

} // namespace qsim
