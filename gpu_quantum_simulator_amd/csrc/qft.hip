// qft.hip — one pass of the quantum Fourier transform: the DFT over one digit of at most ten bits of the register, the twiddle
// factors towards the digits still to come folded into its stores (gfx950).  Its own object, like permutation.hip: nothing here is
// compiled into kernels.hip.  qft.h has the pass rule and the record the host hands over, qft.cpp the host side.
//
// k_qft.  A workgroup walks tiles t = blockIdx.x, + gridDim.x, ... (a static assignment), permutation.hip's walk.  Thread `tid` owns
// the tile-local indices j kTPB + tid on the way in and on the way out, the same in every tile: its part of their addresses, LDS
// slots, u and r is formed once from the record's per-bit tables, the part of j comes off scalar registers.  Per tile it
//   1. has loaded its elements (consecutive threads on consecutive tile-local indices) and writes each into LDS at slot
//      (padding, t): the digit value t on the slot's low d bits (inverse: conjugated, so that everything below runs forwards);
//   2. runs the butterflies in ROUNDS of G = 4 (fp64) or 5 (fp32) slot bits: a thread reads the 2^G slots that differ in the bits
//      [rG, rG + G), applies the radix-2 decimation-in-frequency stages of those bits that lie inside the digit in registers, and
//      writes them back where they were; one barrier per round, ceil(d / G) rounds, the top one first.  A stage's twiddle is
//      exp(2 pi i (t mod 2^b) / 2^(b+1)): a constant 32nd root of unity for the bits inside the round times a factor of the thread's own
//      lower bits, which it keeps in registers (sincospi of an exact fraction in fp64, once per launch);
//   3. reads X[u] from the bit-reversed slot for each of its output indices, multiplies by 2^(-d/2) w^(r u), w = exp(2 pi i / 2^k_p),
//      and stores it at the output address: the digit's qubits for a pass that moves nothing, the low end of the sub-register in the
//      other buffer for one that does.  w^(r u) is a product of three factors, each sincospi of an exact fraction (an integer product
//      below 2^40 mod 2^k_p, over 2^(k_p - 1)) in fp64: the element's own (its r and u bits inside the tile; kept in registers in the
//      state's precision), the thread's per tile (r of the tile's base times its own u bits) and a uniform one per tile and j (lane j
//      of a wave forms it, the others read it off that lane); the last two are multiplied in fp64 and rounded once.  Two sincospi per
//      thread and tile, not one per element;
//   4. waits at a barrier before the next tile's LDS writes.
// The NEXT tile's loads are issued right behind the first barrier, into the registers step 1 has emptied, so they are under way
// while the rounds compute; the stores of step 3 need no waiting for.
// Every output amplitude is formed by one thread in a fixed order: equal calls give equal bits whatever the grid.
// FULL: the tile has qft_tile_bits.  !FULL: one tile of p.elems elements, the whole register; loads and stores are guarded, the
// slots of the elements that are not there hold zeros and no butterfly mixes them with the others (their slot bits lie above the digit).
#include "qft.h"

namespace qsim {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <typename R> struct Elem;
template <> struct Elem<double> { using type = f64x2; };
template <> struct Elem<float> { using type = f32x2; };

// exp(2 pi i m / 32), m < 16
constexpr double kC1 = 0.9807852804032304, kS1 = 0.19509032201612825, kC2 = 0.9238795325112867, kS2 = 0.3826834323650898, kC3 = 0.8314696123025452,
                 kS3 = 0.5555702330196022, kC4 = 0.7071067811865476;
__device__ constexpr double kRootRe[16] = {1.0, kC1, kC2, kC3, kC4, kS3, kS2, kS1, 0.0, -kS1, -kS2, -kS3, -kC4, -kC3, -kC2, -kC1};
__device__ constexpr double kRootIm[16] = {0.0, kS1, kS2, kS3, kC4, kC3, kC2, kC1, 1.0, kC1, kC2, kC3, kC4, kS3, kS2, kS1};

// OR (addresses, bits of u and r) or XOR (swizzled LDS slots) of a per-bit table over the set bits [lo, hi) of v
template <typename T, int N>
__device__ __forceinline__ T fold_or(const T (&tab)[N], uint32_t v, int lo, int hi) {
    T r = 0;
#pragma unroll
    for (int i = lo; i < hi; i++)
        if ((v >> i) & 1u) r |= tab[i];
    return r;
}
template <typename T, int N>
__device__ __forceinline__ T fold_xor(const T (&tab)[N], uint32_t v, int lo, int hi) {
    T r = 0;
#pragma unroll
    for (int i = lo; i < hi; i++)
        if ((v >> i) & 1u) r ^= tab[i];
    return r;
}

// v of lane `lane` of the wave (uniform, a constant once the loops are unrolled)
__device__ __forceinline__ double lane_value(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// The stages of one round on the 2^G values a thread holds: bit s of the position j in (xr, xi) is slot bit l0 + s, and the stages of
// the bits below d run, the highest first.  (twr, twi)[s] = exp(2 pi i low / 2^(l0 + s + 1)), low the thread's slot bits below l0.
template <typename R, int G>
__device__ __forceinline__ void round_stages(R (&xr)[1 << G], R (&xi)[1 << G], const R (&twr)[G], const R (&twi)[G], int l0, int d) {
#pragma unroll
    for (int s = G - 1; s >= 0; s--) {
        if (l0 + s >= d) continue; // uniform
        R cr[1 << (G - 1)], ci[1 << (G - 1)];
#pragma unroll
        for (int jl = 0; jl < (1 << s); jl++) {
            const int m = jl << (4 - s); // exp(2 pi i jl / 2^(s+1)) as a 32nd root
            if (m == 0) cr[jl] = twr[s], ci[jl] = twi[s];
            else if (m == 8) cr[jl] = -twi[s], ci[jl] = twr[s];
            else cr[jl] = twr[s] * (R)kRootRe[m] - twi[s] * (R)kRootIm[m], ci[jl] = twr[s] * (R)kRootIm[m] + twi[s] * (R)kRootRe[m];
        }
#pragma unroll
        for (int j = 0; j < (1 << G); j++) {
            if ((j >> s) & 1) continue;
            const int jh = j | (1 << s), jl = j & ((1 << s) - 1);
            const R ar = xr[j], ai = xi[j], br = xr[jh], bi = xi[jh];
            xr[j] = ar + br, xi[j] = ai + bi;
            const R dr = ar - br, di = ai - bi;
            xr[jh] = dr * cr[jl] - di * ci[jl];
            xi[jh] = dr * ci[jl] + di * cr[jl];
        }
    }
}

template <typename R, bool FULL>
__global__ __launch_bounds__(kTPB) void k_qft(const R *src, R *dst, CtrlGeom g, const QftPassRec *__restrict__ rec) {
    const QftPassRec &p = *rec; // uniform loads of read-only memory: scalar, and a dynamic index needs no copy
    using E = typename Elem<R>::type;
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int G = qft_round_bits(F32), PT = 1 << G, TB = qft_tile_bits(F32), ROUNDS = (kQftMaxDigitBits + G - 1) / G;
    static_assert(kTidBits + G == TB && ROUNDS * G <= TB, "a thread's 2^G elements and the workgroup's threads are the tile; the rounds stay inside it");
    __shared__ E lds[1 << TB]; // 64 KiB
    const E *const a = reinterpret_cast<const E *>(src);
    E *const o = reinterpret_cast<E *>(dst);
    uint32_t tid = threadIdx.x;
    const int d = p.d;
    const uint32_t conj = p.inverse;

    // the thread's own part of every map: the index bits [0, kTidBits)
    uint64_t in_lo = fold_or(p.in_addr, tid, 0, kTidBits), out_lo = fold_or(p.out_addr, tid, 0, kTidBits), r_lo = fold_or(p.out_r, tid, 0, kTidBits);
    uint32_t in_slot_lo = fold_xor(p.in_lds, tid, 0, kTidBits), out_slot_lo = fold_xor(p.out_lds, tid, 0, kTidBits);
    uint32_t u_lo = fold_or(p.out_u, tid, 0, kTidBits);

    // the thread's twiddles, round by round: its slot bits below the round's are its lowest thread bits
    R twr[ROUNDS][G], twi[ROUNDS][G];
#pragma unroll
    for (int r = 0; r < ROUNDS; r++)
#pragma unroll
        for (int s = 0; s < G; s++) {
            const int l0 = r * G;
            double sn = 0.0, cs = 1.0;
            if (l0 > 0 && l0 + s < d) sincospi((double)(tid & ((1u << l0) - 1u)) / (double)(1u << (l0 + s)), &sn, &cs);
            twr[r][s] = (R)cs, twi[r][s] = (R)sn;
        }

    const uint64_t tiles = g.units, kmask = (1ULL << p.kp) - 1ULL;
    const double to_turns = 1.0 / (double)(1ULL << (p.kp > 0 ? p.kp - 1 : 0)); // (r u mod 2^kp) / 2^(kp-1): the argument of sincospi
    const bool twiddle = p.nr > 0;
    // w^(r u) of an output element, r = r_base | r_own and u = u_lo | u_hi(j), as a product of three factors, each sincospi of an exact
    // fraction in fp64: w^(r_own u), the same in every tile, kept here per element; w^(r_base u_lo), one per thread and tile; and
    // w^(r_base u_hi(j)), uniform, which lane j of every wave forms per tile and the others read from it.
    R own_re[PT], own_im[PT];
#pragma unroll
    for (int j = 0; j < PT; j++) {
        double sn = 0.0, cs = 1.0;
        if (twiddle) { // uniform
            const uint32_t w = (uint32_t)j * kTPB;
            const uint64_t r = r_lo | fold_or(p.out_r, w, kTidBits, TB), u = u_lo | fold_or(p.out_u, w, kTidBits, TB);
            sincospi((double)((r * u) & kmask) * to_turns, &sn, &cs);
        }
        own_re[j] = (R)cs, own_im[j] = (R)sn;
    }
    const uint64_t u_hi_of_lane = fold_or(p.out_u, (tid & (uint32_t)(PT - 1)) * kTPB, kTidBits, TB);
    uint64_t t = blockIdx.x;
    if (t >= tiles) return; // uniform
    uint64_t base = spread<double>(g, t);
    E v[PT];
#pragma unroll
    for (int j = 0; j < PT; j++) {
        const uint32_t w = (uint32_t)j * kTPB;
        v[j] = FULL || (w | tid) < p.elems ? a[base | in_lo | fold_or(p.in_addr, w, kTidBits, TB)] : E{0, 0};
    }
    for (;;) {
        // The thread's parts are opaque from here on: what is derived from them (an address or slot per j, one OR or XOR each) is
        // formed where it is used, not once in front of the loop, where it would hold a hundred registers for the whole walk.
        asm volatile("" : "+v"(tid), "+v"(in_lo), "+v"(out_lo), "+v"(r_lo), "+v"(in_slot_lo), "+v"(out_slot_lo), "+v"(u_lo));
#pragma unroll
        for (int j = 0; j < PT; j++) {
            E e = v[j];
            if (conj) e.y = -e.y;
            lds[in_slot_lo ^ fold_xor(p.in_lds, (uint32_t)j * kTPB, kTidBits, TB)] = e;
        }
        __syncthreads();
        // the next tile's loads, into the registers the LDS writes have just emptied: they are under way while the rounds compute
        const uint64_t next = t + gridDim.x;
        const bool more = next < tiles;
        const uint64_t next_base = more ? spread<double>(g, next) : 0;
        if (more) {
#pragma unroll
            for (int j = 0; j < PT; j++) {
                const uint32_t w = (uint32_t)j * kTPB;
                if (FULL || (w | tid) < p.elems) v[j] = a[next_base | in_lo | fold_or(p.in_addr, w, kTidBits, TB)];
            }
        }
#pragma unroll
        for (int r = ROUNDS - 1; r >= 0; r--) {
            const int l0 = r * G;
            if (l0 >= d) continue; // uniform: the digit ends below this round
            const uint32_t mine = qft_swizzle(((tid >> l0) << (l0 + G)) | (tid & ((1u << l0) - 1u)), G);
            R xr[PT], xi[PT];
#pragma unroll
            for (int j = 0; j < PT; j++) {
                const E e = lds[mine ^ qft_swizzle((uint32_t)j << l0, G)];
                xr[j] = e.x, xi[j] = e.y;
            }
            round_stages<R, G>(xr, xi, twr[r], twi[r], l0, d);
#pragma unroll
            for (int j = 0; j < PT; j++) lds[mine ^ qft_swizzle((uint32_t)j << l0, G)] = E{xr[j], xi[j]};
            __syncthreads();
        }
        // where the tile goes and the bits of r it has outside itself: every bit of r moves from r_from to r_to (uniform)
        uint64_t out_base = base & ~p.sub_mask, r_base = 0;
        for (int i = 0; i < p.nr; i++) {
            const uint64_t bit = (base >> p.r_from[i]) & 1ULL;
            r_base |= bit << i;
            out_base |= bit << p.r_to[i];
        }
        double c_re = p.scale, c_im = 0.0, lane_re = 1.0, lane_im = 0.0;
        if (twiddle) { // uniform
            double sn, cs;
            sincospi((double)((r_base * (uint64_t)u_lo) & kmask) * to_turns, &sn, &cs);
            c_re = cs * p.scale, c_im = sn * p.scale;
            sincospi((double)((r_base * u_hi_of_lane) & kmask) * to_turns, &lane_im, &lane_re);
        }
#pragma unroll
        for (int j = 0; j < PT; j++) {
            const uint32_t w = (uint32_t)j * kTPB;
            const E e = lds[out_slot_lo ^ fold_xor(p.out_lds, w, kTidBits, TB)];
            R fr = (R)c_re, fi = (R)c_im;
            if (twiddle) { // uniform: the product in fp64, rounded once, times the element's own factor in the state's precision
                const double q_re = lane_value(lane_re, j), q_im = lane_value(lane_im, j);
                const R t_re = (R)(c_re * q_re - c_im * q_im), t_im = (R)(c_re * q_im + c_im * q_re);
                fr = t_re * own_re[j] - t_im * own_im[j], fi = t_re * own_im[j] + t_im * own_re[j];
            }
            E f{e.x * fr - e.y * fi, e.x * fi + e.y * fr};
            if (conj) f.y = -f.y;
            if (FULL || (w | tid) < p.elems) o[out_base | out_lo | fold_or(p.out_addr, w, kTidBits, TB)] = f;
        }
        if (!more) break;
        __syncthreads(); // every output read is done before the next tile's LDS writes
        t = next, base = next_base;
    }
}

template <typename R, bool FULL>
hipError_t launch_shape(const LaunchCfg &cfg, const void *src, void *dst, const CtrlGeom &g, const QftPassRec *d_rec) {
    unsigned grid = writing_grid<k_qft<R, FULL>>(cfg, g.units, 1);
    if (cfg.grid_cap <= 0 && grid > (unsigned)kQftGridCap) grid = (unsigned)kQftGridCap;
    hipLaunchKernelGGL((k_qft<R, FULL>), dim3(grid), dim3(kTPB), 0, cfg.stream, (const R *)src, (R *)dst, g, d_rec);
    return hipGetLastError();
}

} // namespace

hipError_t launch_qft_pass(const LaunchCfg &cfg, const void *src, void *dst, const QftPlan &plan, int p, const QftPassRec &rec, const QftPassRec *d_rec) {
    if (!src || !dst || !d_rec || plan.n < 0 || plan.n > 40 || p < 0 || p >= plan.passes) return hipErrorInvalidValue;
    const QftPass &ps = plan.pass[p];
    const uint64_t all = index_mask(plan.n);
    const int full_bits = qft_tile_bits(plan.f32);
    // every address is spread(tile) | (its r bits moved) | a fold of the record's per-bit tables: inside the buffer when the tables
    // hold tile_bits distinct single qubits of the register each, and the r bits move inside the sub-register
    if (ps.tile_bits < 0 || ps.tile_bits > full_bits || ps.tile_bits > plan.n || ps.tile_bits != __builtin_popcountll(ps.in_mask) ||
        ps.tile_bits != __builtin_popcountll(ps.out_mask) || ((ps.in_mask | ps.out_mask | rec.sub_mask) & ~all))
        return hipErrorInvalidValue;
    if (rec.d != ps.d || rec.kp != ps.kp || rec.nr != ps.kp - ps.d || rec.d < 1 || rec.d > kQftMaxDigitBits || rec.d > ps.tile_bits || rec.kp > plan.n ||
        rec.elems != 1u << ps.tile_bits)
        return hipErrorInvalidValue;
    uint64_t in_seen = 0, out_seen = 0;
    uint32_t in_slots = 0, out_slots = 0;
    for (int i = 0; i < kQftMaxTileBits; i++) {
        const bool live = i < ps.tile_bits;
        if (live != (rec.in_addr[i] != 0) || live != (rec.out_addr[i] != 0)) return hipErrorInvalidValue;
        if (live && (__builtin_popcountll(rec.in_addr[i]) != 1 || __builtin_popcountll(rec.out_addr[i]) != 1)) return hipErrorInvalidValue;
        if ((in_seen & rec.in_addr[i]) || (out_seen & rec.out_addr[i])) return hipErrorInvalidValue;
        in_seen |= rec.in_addr[i], out_seen |= rec.out_addr[i];
        if (i < full_bits) { // the slots: qft_swizzle of distinct single bits below the tile's size
            const int G = qft_round_bits(plan.f32);
            bool in_ok = false, out_ok = false;
            for (int b = 0; b < full_bits; b++) {
                if (rec.in_lds[i] == qft_swizzle(1u << b, G) && !((in_slots >> b) & 1u)) in_ok = true, in_slots |= 1u << b;
                if (rec.out_lds[i] == qft_swizzle(1u << b, G) && !((out_slots >> b) & 1u)) out_ok = true, out_slots |= 1u << b;
            }
            if (!in_ok || !out_ok) return hipErrorInvalidValue;
        }
    }
    if (in_seen != ps.in_mask || out_seen != ps.out_mask) return hipErrorInvalidValue;
    uint64_t to_seen = 0;
    for (int i = 0; i < rec.nr; i++) {
        if (rec.r_from[i] >= plan.n || rec.r_to[i] >= plan.n || !((rec.sub_mask >> rec.r_from[i]) & 1ULL) || !((rec.sub_mask >> rec.r_to[i]) & 1ULL) ||
            ((to_seen >> rec.r_to[i]) & 1ULL))
            return hipErrorInvalidValue;
        to_seen |= 1ULL << rec.r_to[i];
    }
    if (rec.nr > 0 && src == dst) return hipErrorInvalidValue; // a pass that moves bits is not closed over its tile
    if ((src == dst) != !ps.oop) return hipErrorInvalidValue;
    const CtrlGeom g = ctrl_geom(ps.in_mask, 0, false, plan.n);
    const bool full = ps.tile_bits == full_bits;
    if (g.units != plan.tiles || g.units != 1ULL << (plan.n - ps.tile_bits) || (!full && g.units != 1)) return hipErrorInvalidValue;
    if (plan.f32) return full ? launch_shape<float, true>(cfg, src, dst, g, d_rec) : launch_shape<float, false>(cfg, src, dst, g, d_rec);
    return full ? launch_shape<double, true>(cfg, src, dst, g, d_rec) : launch_shape<double, false>(cfg, src, dst, g, d_rec);
}

} // namespace qsim
