// permutation.hip — a permutation of the basis states of up to ten target qubits, under any number of controls, as ONE in-place
// sweep of the control subspace (gfx950).  Its own object, like matrix.hip: nothing here is compiled into kernels.hip.
// permutation.h has the tile rule and the operand, permutation.cpp the host side; this file has the kernel.
//
// k_permutation.  A workgroup walks tiles t = blockIdx.x, + gridDim.x, ... (a static assignment).  Thread `tid` owns the tile-local
// indices u = j kTPB + tid, the same in every tile: it reads their destinations from the map once and keeps them in registers, and
// forms their address bits deposit(u, tile mask) once.  Per tile it
//   1. has loaded its elements base | at[j] — consecutive threads on consecutive tile-local indices, so as coalesced as the tile is;
//   2. writes each into LDS at its destination (the only scattered step, and it is LDS that takes it);
//   3. waits at a barrier;
//   4. issues the NEXT tile's loads into the registers step 2 has just emptied, then reads LDS linearly and stores to the addresses
//      it loaded — the tile's own, so nothing is written that another workgroup reads;
//   5. waits at a second barrier before the next tile's LDS writes.
// Nothing is computed: an amplitude's bits arrive as they left, in fp64 and in fp32, and each is written by one thread whatever
// the grid is.  An element is one amplitude (16 bytes fp64, 8 bytes fp32): qubit 0 may be a target or a control in fp32 like any
// other, and there is no unit path that moves two fp32 slots as one.
// FULL: the tile has perm_tile_bits and every thread its perm_per_thread elements, no guard.  !FULL: one tile of `elems` < that many
// elements, the whole control subspace of a small register, every access guarded by u < elems.
#include "permutation.h"

namespace qsim {
namespace {

// one amplitude as a native vector: what moves is 16 or 8 bytes, never a (re, im) pair of fields
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <typename R> struct Elem;
template <> struct Elem<double> { using type = f64x2; };
template <> struct Elem<float> { using type = f32x2; };

template <typename R, bool FULL>
__global__ __launch_bounds__(kTPB) void k_permutation(R *amp, CtrlGeom g, uint64_t tile_mask, uint32_t elems, const uint16_t *__restrict__ map) {
    using E = typename Elem<R>::type;
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int PT = perm_per_thread(F32);
    __shared__ E lds[1 << perm_tile_bits(F32)]; // 64 KiB
    E *const a = reinterpret_cast<E *>(amp);
    const uint32_t tid = threadIdx.x;

    uint32_t dst[PT];
    uint64_t at[PT];
#pragma unroll
    for (int j = 0; j < PT; j++) {
        const uint32_t u = (uint32_t)j * kTPB + tid;
        dst[j] = FULL || u < elems ? map[u] : 0u;
        at[j] = deposit(u, tile_mask) | g.ones;
    }

    const uint64_t tiles = g.units;
    uint64_t t = blockIdx.x;
    if (t >= tiles) return; // uniform
    uint64_t base = spread<double>(g, t); // amplitudes, not units: the fp64 shape in both precisions
    E v[PT];
#pragma unroll
    for (int j = 0; j < PT; j++)
        if (FULL || (uint32_t)j * kTPB + tid < elems) v[j] = a[base | at[j]];
    for (;;) {
#pragma unroll
        for (int j = 0; j < PT; j++)
            if (FULL || (uint32_t)j * kTPB + tid < elems) lds[dst[j]] = v[j];
        __syncthreads();
        const uint64_t next = t + gridDim.x;
        const bool more = next < tiles;
        const uint64_t next_base = more ? spread<double>(g, next) : 0;
        if (more) {
#pragma unroll
            for (int j = 0; j < PT; j++)
                if (FULL || (uint32_t)j * kTPB + tid < elems) v[j] = a[next_base | at[j]];
        }
#pragma unroll
        for (int j = 0; j < PT; j++)
            if (FULL || (uint32_t)j * kTPB + tid < elems) a[base | at[j]] = lds[(uint32_t)j * kTPB + tid];
        if (!more) break;
        __syncthreads(); // every linear read is done before the next tile's scattered writes
        t = next, base = next_base;
    }
}

template <typename R, bool FULL>
hipError_t launch_shape(const LaunchCfg &cfg, void *amps, const PermutationPlan &p, const CtrlGeom &g, const uint16_t *d_map) {
    unsigned grid = writing_grid<k_permutation<R, FULL>>(cfg, g.units, 1);
    if (cfg.grid_cap <= 0 && grid > (unsigned)kPermGridCap) grid = (unsigned)kPermGridCap;
    hipLaunchKernelGGL((k_permutation<R, FULL>), dim3(grid), dim3(kTPB), 0, cfg.stream, (R *)amps, g, p.mask, 1u << p.tile_bits, d_map);
    return hipGetLastError();
}

} // namespace

hipError_t launch_permutation(const LaunchCfg &cfg, void *amps, const PermutationPlan &p, const uint16_t *d_map) {
    const uint64_t all = index_mask(p.n);
    if (!amps || !d_map || p.n < 0 || p.n > 40 || ((p.mask | p.controls) & ~all) || (p.mask & p.controls)) return hipErrorInvalidValue;
    // every address is spread(tile) | controls | deposit(tile-local index): inside the buffer when the three bit sets are disjoint,
    // inside the register, and together all of it
    const int full_bits = perm_tile_bits(p.f32), c = __builtin_popcountll(p.controls);
    if (p.tile_bits != __builtin_popcountll(p.mask) || p.tile_bits < 0 || p.tile_bits > full_bits || c != p.num_controls) return hipErrorInvalidValue;
    CtrlGeom g = ctrl_geom(p.mask | p.controls, 0, false, p.n);
    g.ones = p.controls;
    if (g.units != p.tiles || p.n - c - p.tile_bits < 0 || g.units != 1ULL << (p.n - c - p.tile_bits)) return hipErrorInvalidValue;
    const bool full = p.tile_bits == full_bits;
    if (full != (p.path == 1) || (!full && g.units != 1)) return hipErrorInvalidValue;
    if (p.f32) return full ? launch_shape<float, true>(cfg, amps, p, g, d_map) : launch_shape<float, false>(cfg, amps, p, g, d_map);
    return full ? launch_shape<double, true>(cfg, amps, p, g, d_map) : launch_shape<double, false>(cfg, amps, p, g, d_map);
}

} // namespace qsim
