// sample.hip — drawing basis states of a whole register on the device (gfx950; sample.h has the pyramid):
//     k_sample_chunk_sums   one read-only sweep: every wave scans chunks of 256 amplitudes and stores each chunk's total
//     k_sample_prefix       the chunk totals -> running sums inside each group (W), the group totals -> running sums (T); sequential chains
//     k_sample_draws        one wave per draw: bisect T, bisect the group's W, scan the chunk again, ballot for the index
// Its own object, like diagonal.hip: nothing here is compiled into kernels.hip.  sample.cpp is the host side.
//
// chunk_scan is the ONE function that turns a chunk into cumulative sums, in a fixed order: trip j of a wave takes amplitude 64 j + lane
// (consecutive lanes on consecutive amplitudes: 16 bytes per lane in fp64, 8 in fp32), p = fma(re, re, im im) on widened components as
// k_block_prob forms it, an inclusive scan over the wave per trip (doubling steps inside each row of 16 lanes through DPP, then the three
// row totals read off lanes 15, 31 and 47), and the trips chained through lane 63.  The sweep stores the scan's LAST value as the chunk's
// total and the draws run the same function on the same values, so what the pyramid says a chunk adds is what its scan ends on.
// A parallel scan need not be monotone along the lanes; nothing below needs that: the draws take the FIRST lane that qualifies.
//
// No atomics; every output is written by one lane.  No LDS but the staging tile of k_sample_prefix, whose workgroup is one wave.
#include "sample.h"

namespace qsim {
namespace {

template <typename R> struct Amp;
template <> struct Amp<double> { using type = double2; };
template <> struct Amp<float> { using type = float2; };

// the value of the lane CTRL names (a DPP control: 0x110 + k is row_shr:k), 0.0 where that lane lies outside the row of 16
template <int CTRL>
__device__ __forceinline__ double dpp_or_zero(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// lane `src` of v, uniform over the wave (through a scalar register)
__device__ __forceinline__ double read_lane(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
// inclusive scan over the 64 lanes, in this order: inside each row of 16 lanes by doubling steps, then the totals of the rows below, added
// left to right, on top.  Every lane of the wave must get here.
__device__ __forceinline__ double wave_scan(double v, uint32_t lane) {
    v += dpp_or_zero<0x111>(v);
    v += dpp_or_zero<0x112>(v);
    v += dpp_or_zero<0x114>(v);
    v += dpp_or_zero<0x118>(v);
    const double t0 = read_lane(v, 15), t1 = read_lane(v, 31), t2 = read_lane(v, 47);
    const double t01 = t0 + t1, t012 = t01 + t2;
    const uint32_t row = lane >> 4;
    const double below = row == 0 ? 0.0 : row == 1 ? t0 : row == 2 ? t01 : t012;
    return below + v;
}

// p[j] = |a|^2 of amplitude first + 64 j + lane.  PLAIN: a register smaller than a chunk (n < 8) — amplitudes at or beyond `amps` are
// not loaded and count as zero.
// In two steps, so that the sweep can leave the loads of its next chunk in flight behind the scan of this one: chunk_fetch issues them,
// chunk_probs is their first use.
template <typename R, bool PLAIN>
__device__ __forceinline__ void chunk_fetch(const R *__restrict__ a, uint64_t first, uint64_t amps, uint32_t lane, typename Amp<R>::type (&v)[kSampleTrips]) {
    using P = typename Amp<R>::type;
#pragma unroll
    for (int j = 0; j < kSampleTrips; j++) {
        const uint64_t i = first + 64u * j + lane;
        v[j] = P{};
        if (!PLAIN || i < amps) v[j] = *reinterpret_cast<const P *>(a + 2 * i);
    }
}
template <typename P>
__device__ __forceinline__ void chunk_probs(const P (&v)[kSampleTrips], double (&p)[kSampleTrips]) {
#pragma unroll
    for (int j = 0; j < kSampleTrips; j++) p[j] = fma((double)v[j].x, (double)v[j].x, (double)v[j].y * (double)v[j].y);
}
template <typename R, bool PLAIN>
__device__ __forceinline__ void chunk_load(const R *__restrict__ a, uint64_t first, uint64_t amps, uint32_t lane, double (&p)[kSampleTrips]) {
    typename Amp<R>::type v[kSampleTrips];
    chunk_fetch<R, PLAIN>(a, first, amps, lane, v);
    chunk_probs(v, p);
}
// s[j] = the cumulative sum of the chunk up to and including amplitude 64 j + lane; returns the chunk's total: s[last] of lane 63
__device__ __forceinline__ double chunk_scan(const double (&p)[kSampleTrips], uint32_t lane, double (&s)[kSampleTrips]) {
    double carry = 0.0;
#pragma unroll
    for (int j = 0; j < kSampleTrips; j++) {
        s[j] = carry + wave_scan(p[j], lane);
        carry = read_lane(s[j], 63);
    }
    return carry;
}

// ---- 1. the sweep -----------------------------------------------------------------------------------------------------------------
// Wave w of the grid takes chunks w, w + waves, ...; the loads of the next chunk are issued before the scan of this one.
template <typename R>
__global__ __launch_bounds__(kTPB) void k_sample_chunk_sums(const R *__restrict__ a, SampleGeom g, double *__restrict__ w) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double p[kSampleTrips], s[kSampleTrips];

    if (g.chunk_bits < kSampleChunkBits) { // the plain path: the register is one chunk, one wave scans what there is of it
        if (blockIdx.x == 0 && wave == 0) {
            chunk_load<R, true>(a, 0, g.amps, lane, p);
            const double total = chunk_scan(p, lane, s);
            if (lane == 0) w[0] = total;
        }
        return;
    }

    const uint64_t stride = (uint64_t)gridDim.x * kSampleWaves;
    uint64_t c = (uint64_t)blockIdx.x * kSampleWaves + wave;
    if (c >= g.chunks) return; // uniform over the wave; no barrier follows
    typename Amp<R>::type cur[kSampleTrips], nxt[kSampleTrips];
    chunk_fetch<R, false>(a, c << kSampleChunkBits, g.amps, lane, cur);
    for (;;) {
        const uint64_t next = c + stride;
        const bool more = next < g.chunks;
        // unconditionally, so that nothing waits for them before the scan: a wave's last trip fetches its own chunk once more
        chunk_fetch<R, false>(a, (more ? next : c) << kSampleChunkBits, g.amps, lane, nxt);
        chunk_probs(cur, p);
        const double total = chunk_scan(p, lane, s);
        if (lane == 0) w[c] = total;
        if (!more) break;
        for (int j = 0; j < kSampleTrips; j++) cur[j] = nxt[j];
        c = next;
    }
}

// ---- 2. the running sums ----------------------------------------------------------------------------------------------------------
// v[t * len + i] <- v[t * len] + ... + v[t * len + i], added one after the other in ascending i by ONE lane: a sequential sum of
// non-negative terms never decreases, a tree of partial sums may.  A workgroup is one wave; it stages a tile of `len` <= 1024 entries
// through LDS so that the global accesses are the wave's and the chain runs on LDS.  chained == 0: every tile starts at zero and
// totals[t] gets its last value (the groups of W).  chained != 0: ONE workgroup, a tile starts where the one before it ended (T).
__global__ __launch_bounds__(64) void k_sample_prefix(double *v, uint64_t tiles, uint32_t len, double *__restrict__ totals, int chained) {
    __shared__ double tile[kSamplePrefixTile];
    const uint32_t lane = threadIdx.x;
    double carry = 0.0; // lane 0's
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        double *p = v + t * len;
        for (uint32_t i = lane; i < len; i += 64) tile[i] = p[i];
        __syncthreads();
        if (lane == 0) {
            double acc = chained ? carry : 0.0;
#pragma unroll 8
            for (uint32_t i = 0; i < len; i++) {
                acc += tile[i];
                tile[i] = acc;
            }
            carry = acc;
            if (!chained) totals[t] = acc;
        }
        __syncthreads();
        for (uint32_t i = lane; i < len; i += 64) p[i] = tile[i];
        __syncthreads(); // the tile is free for the next trip
    }
}

// ---- 3. the draws -----------------------------------------------------------------------------------------------------------------
// The first entry e in [0, count) with base + v[e] > 0 and >= r, count - 1 when rounding leaves none: never outside the array.
__device__ __forceinline__ uint64_t first_reaching(const double *__restrict__ v, uint64_t count, double base, double r) {
    uint64_t lo = 0, hi = count - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const double c = base + v[mid];
        if (c > 0.0 && c >= r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

template <typename R>
__global__ __launch_bounds__(kTPB) void k_sample_draws(const R *__restrict__ a, SampleGeom g, const double *__restrict__ w, const double *__restrict__ t,
                                                      const double *__restrict__ draws, uint64_t shots, SampleQubits qs, uint64_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double total = t[g.groups - 1];
    const uint64_t group_chunks = 1ULL << g.group_chunk_bits;
    for (uint64_t k = (uint64_t)blockIdx.x * kSampleWaves + wave; k < shots; k += (uint64_t)gridDim.x * kSampleWaves) { // uniform over the wave
        const double r = draws[k] * total;
        const uint64_t gi = first_reaching(t, g.groups, 0.0, r);
        const double below_group = gi ? t[gi - 1] : 0.0;
        const double *wg = w + (gi << g.group_chunk_bits);
        const uint64_t ci = first_reaching(wg, group_chunks, below_group, r);
        const double base = below_group + (ci ? wg[ci - 1] : 0.0);
        const uint64_t first = ((gi << g.group_chunk_bits) | ci) << g.chunk_bits;

        double p[kSampleTrips], s[kSampleTrips];
        if (g.chunk_bits < kSampleChunkBits) chunk_load<R, true>(a, first, g.amps, lane, p);
        else chunk_load<R, false>(a, first, g.amps, lane, p);
        (void)chunk_scan(p, lane, s);

        // the first index of the chunk with p > 0 whose cumulative value is non-zero and reaches r; base + s of the chunk's end and the
        // bisected below_group + W round differently, so there may be none: then the chunk's last index with p > 0 (there is one: the
        // chunk is the first to reach r, so W grew across it)
        int hit = -1, last = (1 << g.chunk_bits) - 1;
#pragma unroll
        for (int j = 0; j < kSampleTrips; j++) {
            const unsigned long long live = __ballot(p[j] > 0.0);
            if (live) last = 64 * j + 63 - __builtin_clzll(live);
        }
#pragma unroll
        for (int j = kSampleTrips - 1; j >= 0; j--) {
            const double c = base + s[j];
            const unsigned long long reach = __ballot(p[j] > 0.0 && c > 0.0 && c >= r);
            if (reach) hit = 64 * j + __builtin_ctzll(reach);
        }
        const uint64_t index = first + (uint64_t)(hit >= 0 ? hit : last);
        if (lane == 0) {
            uint64_t res = index;
            if (qs.count > 0) {
                res = 0;
                for (int j = 0; j < qs.count; j++) res |= ((index >> qs.q[j]) & 1ULL) << j;
            }
            out[k] = res;
        }
    }
}

// ---- grids: QSIM_OPT_GRID_CAP > 0 caps all three, as it caps the sweeps that only write; no result depends on the grid ----------------
template <auto Kernel>
unsigned capped_grid(int grid_cap, uint64_t blocks) {
    const int resident = resident_grid<Kernel>();
    const uint64_t cap = grid_cap > 0 ? (uint64_t)grid_cap : resident > 0 && resident < kSampleGrid ? (uint64_t)resident : (uint64_t)kSampleGrid;
    if (blocks > cap) blocks = cap;
    return blocks == 0 ? 1u : (unsigned)blocks;
}

template <typename R>
hipError_t launch_chunk_sums_prec(const LaunchCfg &cfg, const void *amps, const SampleGeom &g, double *d_w) {
    const unsigned grid = capped_grid<k_sample_chunk_sums<R>>(cfg.grid_cap, (g.chunks + kSampleWaves - 1) / kSampleWaves);
    hipLaunchKernelGGL((k_sample_chunk_sums<R>), dim3(grid), dim3(kTPB), 0, cfg.stream, (const R *)amps, g, d_w);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_draws_prec(const LaunchCfg &cfg, const void *amps, const SampleGeom &g, const double *d_w, const double *d_t, const double *d_draws,
                             uint64_t shots, const SampleQubits &qubits, uint64_t *d_out) {
    const unsigned grid = capped_grid<k_sample_draws<R>>(cfg.grid_cap, (shots + kSampleWaves - 1) / kSampleWaves);
    hipLaunchKernelGGL((k_sample_draws<R>), dim3(grid), dim3(kTPB), 0, cfg.stream, (const R *)amps, g, d_w, d_t, d_draws, shots, qubits, d_out);
    return hipGetLastError();
}

} // namespace

hipError_t launch_sample_chunk_sums(const LaunchCfg &cfg, const void *amps, bool f32, int n, double *d_w) {
    if (n < 0 || n > 40 || !amps || !d_w) return hipErrorInvalidValue;
    const SampleGeom g = sample_geom(n);
    return f32 ? launch_chunk_sums_prec<float>(cfg, amps, g, d_w) : launch_chunk_sums_prec<double>(cfg, amps, g, d_w);
}

hipError_t launch_sample_prefix(const LaunchCfg &cfg, int n, double *d_w, double *d_t) {
    if (n < 0 || n > 40 || !d_w || !d_t) return hipErrorInvalidValue;
    const SampleGeom g = sample_geom(n);
    // the groups of W, a tile each, in parallel
    const uint64_t cap = cfg.grid_cap > 0 ? (uint64_t)cfg.grid_cap : 4096;
    const unsigned grid = (unsigned)(g.groups < cap ? g.groups : cap);
    hipLaunchKernelGGL(k_sample_prefix, dim3(grid), dim3(64), 0, cfg.stream, d_w, g.groups, 1u << g.group_chunk_bits, d_t, 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // T: one chain over the groups' totals, tile after tile in one workgroup
    const uint64_t len = g.groups < (uint64_t)kSamplePrefixTile ? g.groups : (uint64_t)kSamplePrefixTile;
    hipLaunchKernelGGL(k_sample_prefix, dim3(1), dim3(64), 0, cfg.stream, d_t, g.groups / len, (uint32_t)len, (double *)nullptr, 1);
    return hipGetLastError();
}

hipError_t launch_sample_draws(const LaunchCfg &cfg, const void *amps, bool f32, int n, const double *d_w, const double *d_t, const double *d_draws,
                               long shots, const SampleQubits &qubits, uint64_t *d_out) {
    if (n < 0 || n > 40 || !amps || !d_w || !d_t || !d_draws || !d_out || shots < 1 || qubits.count < 0 || qubits.count > kSampleMaxQubits)
        return hipErrorInvalidValue;
    const SampleGeom g = sample_geom(n);
    return f32 ? launch_draws_prec<float>(cfg, amps, g, d_w, d_t, d_draws, (uint64_t)shots, qubits, d_out)
               : launch_draws_prec<double>(cfg, amps, g, d_w, d_t, d_draws, (uint64_t)shots, qubits, d_out);
}

} // namespace qsim
