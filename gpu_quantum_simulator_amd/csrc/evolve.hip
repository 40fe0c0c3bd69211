// evolve.hip — Pauli-string rotations exp(-i theta/2 P) as in-place sweeps (gfx950).  Its own object, like expect.hip: nothing
// here is compiled into kernels.hip, whose code layout is part of the measured product.
//
// A string is two masks: x (bit q: X or Y on qubit q) and z (bit q: Z or Y).  P maps every index pair {j, j ^ x} to itself, so
// the rotation is a 2x2 on each pair whatever the string's weight.  With s(j) = (-1)^popcount(j & z), ny = popcount(x & z),
// c = cos(theta/2) and w = -i sin(theta/2) i^ny:
//     a_j'       = c a_j       + w (-1)^ny s(j) b_(j^x)
//     b_(j^x)'   = c b_(j^x)   + w s(j) a_j
// w is real for odd ny and imaginary for even ny, so the host hands over c and ONE real number v per term (w = v or w = i v) and
// a bit that says which; the device selects signs and never sees an angle.  x == 0 is the diagonal case of the same rule
// (b = a, ny = 0): a_j' = (c + i v s(j)) a_j with v = -sin(theta/2).
// Consecutive terms that share x map the same pairs to themselves: a run of up to kMaxRotTermsPerSweep of them is applied in
// registers, in the caller's order, between one load and one store of the state.
//
// Work is dealt in UNITS of 16 bytes per lane, exactly as in k_expect: one fp64 amplitude or two fp32 amplitudes, consecutive
// lanes on consecutive units; the partner unit (j ^ x) permutes the same 128-byte lines.  A unit index t = (q << 8) | tid is
// expanded to an amplitude index by a bit insertion (the zero at the highest bit of x), which is linear over OR of disjoint bit
// sets: popcount(j & z) = popcount(E(q << 8) & z) + popcount(E(tid) & z) (+ z bit 0 for the odd fp32 slot).  The first part is
// uniform over the workgroup (scalar unit, per unit and term), the second is one bit per term and thread, formed once before the
// loop.  Every amplitude is written by exactly one thread: no atomics, no reduction, equal calls give equal bits.
#include "qsim_internal.h"

namespace qsim {
namespace {

constexpr int kTPB = 256;                     // 4 waves; a unit index's low 8 bits are the thread
constexpr int kTidBits = 8;
static_assert((1 << kTidBits) == kTPB, "unit index = (q << kTidBits) | tid");
constexpr int KT = kMaxRotTermsPerSweep;
static_assert(KT <= 32, "one bit per term in RotTerms::odd and in a thread's parity mask");

template <typename R>
struct RotTerms {       // by value: scalar loads
    uint64_t z[KT];
    R c[KT], v[KT];     // rounded once to the state's precision by the host
    uint32_t odd;       // bit k: ny is odd — w = v is real and a's sign is opposite to b's; else w = i v
    int32_t count;
};
static_assert(sizeof(RotTerms<double>) <= 1024, "term records stay well inside the 4 KiB of kernel arguments");

struct RotGeom {        // the geometry of k_expect's SweepGeom
    uint64_t units;     // 16-byte units to visit
    uint64_t low;       // unit-index bits below the inserted zero (all ones: nothing inserted)
    uint64_t x;         // partner amplitude = amplitude ^ x
    uint64_t amps;      // amplitudes in the buffer (guards the one-amplitude fp32 register)
    uint32_t odd_slot;  // fp32: the odd amplitude of a unit is a pair member of its own (0 only for x == 1 on one state: both members share the unit)
};

template <typename R> struct Vec16;
template <> struct Vec16<double> { using type = double2; };
template <> struct Vec16<float> { using type = float4; };

__device__ __forceinline__ double flip(double v, uint32_t sign_bit31) {
    return __hiloint2double(__double2hiint(v) ^ (int)sign_bit31, __double2loint(v));
}
__device__ __forceinline__ float flip(float v, uint32_t sign_bit31) { return __uint_as_float(__float_as_uint(v) ^ sign_bit31); }

// one pair, sv = s(j) v
template <typename R>
__device__ __forceinline__ void rotate_pair(R &ar, R &ai, R &br, R &bi, R c, R sv, bool odd) {
    const R pr = odd ? br : bi, pi = odd ? bi : br;   // w b = sv (br, bi) or sv (-bi, br); a's sign: -1 for odd ny
    const R qr = odd ? ar : ai, qi = odd ? ai : ar;   // w a likewise
    const R nar = fma(-sv, pr, c * ar), nai = fma(odd ? -sv : sv, pi, c * ai);
    const R nbr = fma(odd ? sv : -sv, qr, c * br), nbi = fma(sv, qi, c * bi);
    ar = nar, ai = nai, br = nbr, bi = nbi;
}
// x == 0: a' = (c + i sv) a
template <typename R>
__device__ __forceinline__ void rotate_diag(R &ar, R &ai, R c, R sv) {
    const R nr = fma(-sv, ai, c * ar), ni = fma(sv, ar, c * ai);
    ar = nr, ai = ni;
}

template <typename R, bool PAIRED>
__global__ __launch_bounds__(kTPB) void k_pauli_rot(R *a, R *b, RotGeom g, RotTerms<R> terms) { // a and b may be one buffer
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2;       // amplitudes per unit
    constexpr int AS = A - 1;
    constexpr int U = PAIRED ? 4 : 8;               // units per thread and trip: 8 independent 16-byte loads in flight
    const uint32_t tid = threadIdx.x;
    const bool two_units = PAIRED && g.odd_slot;    // the partner sits in a unit of its own (else: in the odd slot of a's unit)
    auto expand = [&](uint64_t t) { return (((t & ~g.low) << 1) | (t & g.low)) << AS; }; // unit index -> its (even) amplitude index
    auto load = [&](const R *p, uint64_t amp) -> V { return *reinterpret_cast<const V *>(p + 2 * amp); };
    auto store = [&](R *p, uint64_t amp, const V &v) { *reinterpret_cast<V *>(p + 2 * amp) = v; };

    if constexpr (A == 2) if (g.amps < 2) { // a register of one fp32 amplitude is 8 bytes long, no unit: one thread, 8-byte accesses
        if (blockIdx.x == 0 && tid == 0) {
            float2 one = *reinterpret_cast<const float2 *>(a), two = PAIRED ? *reinterpret_cast<const float2 *>(b) : float2{0.f, 0.f};
            for (int k = 0; k < terms.count; k++) { // no index bit: s(j) = 1
                if (PAIRED) rotate_pair(one.x, one.y, two.x, two.y, terms.c[k], terms.v[k], (terms.odd >> k) & 1u);
                else rotate_diag(one.x, one.y, terms.c[k], terms.v[k]);
            }
            *reinterpret_cast<float2 *>(a) = one;
            if (PAIRED) *reinterpret_cast<float2 *>(b) = two;
        }
        return;
    }

    // the thread's own index bits: one parity bit per term, once
    const uint64_t jl = expand(tid);
    uint32_t own = 0;
    for (int k = 0; k < terms.count; k++) own |= ((uint32_t)__builtin_popcountll(jl & terms.z[k]) & 1u) << k;
    const int slots = (A == 2 && g.odd_slot) ? 2 : 1;

    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.units; q0 += (uint64_t)gridDim.x * U) {
        R ar[U][A], ai[U][A], br[U][A], bi[U][A];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            V va{}, vb{};
            if (t < g.units) {
                const uint64_t j = expand(t);
                va = load(a, j);
                if (two_units) vb = load(b, (j ^ g.x) & ~(uint64_t)AS);
            }
            if constexpr (A == 1) {
                ar[u][0] = va.x, ai[u][0] = va.y;
                br[u][0] = vb.x, bi[u][0] = vb.y;
            } else {
                ar[u][0] = va.x, ai[u][0] = va.y, ar[u][1] = va.z, ai[u][1] = va.w;
                if (PAIRED && !g.odd_slot) vb = V{va.z, va.w, 0.f, 0.f};                   // x == 1 on one state: the pair is the unit
                else if (PAIRED && (g.x & 1)) vb = V{vb.z, vb.w, vb.x, vb.y};              // the partner sits in the other half of its unit
                br[u][0] = vb.x, bi[u][0] = vb.y, br[u][1] = vb.z, bi[u][1] = vb.w;
            }
        }
        for (int k = 0; k < terms.count; k++) { // uniform: the term's record comes through scalar loads
            const uint64_t z = terms.z[k];
            const R c = terms.c[k], v = terms.v[k];
            const bool odd = (terms.odd >> k) & 1u;
            const uint32_t mine = ((own >> k) & 1u) << 31;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t ju = expand((q0 + u) << kTidBits); // uniform part of the amplitude index
                const uint32_t sg = (((uint32_t)__builtin_popcountll(ju & z) & 1u) << 31) ^ mine;
#pragma unroll
                for (int s = 0; s < A; s++) {
                    if (s >= slots) continue;
                    const R sv = flip(v, s ? sg ^ ((uint32_t)(z & 1ULL) << 31) : sg);
                    if (PAIRED) rotate_pair(ar[u][s], ai[u][s], br[u][s], bi[u][s], c, sv, odd);
                    else rotate_diag(ar[u][s], ai[u][s], c, sv);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            if (t >= g.units) continue;
            const uint64_t j = expand(t);
            if constexpr (A == 1) {
                store(a, j, V{ar[u][0], ai[u][0]});
                if (two_units) store(b, j ^ g.x, V{br[u][0], bi[u][0]});
            } else { // selects on values, so that every store stays one 16-byte store
                const bool same = PAIRED && !g.odd_slot, swapped = (g.x & 1) != 0;
                store(a, j, V{ar[u][0], ai[u][0], same ? br[u][0] : ar[u][1], same ? bi[u][0] : ai[u][1]});
                if (two_units)
                    store(b, (j ^ g.x) & ~(uint64_t)AS,
                          V{swapped ? br[u][1] : br[u][0], swapped ? bi[u][1] : bi[u][0], swapped ? br[u][0] : br[u][1], swapped ? bi[u][0] : bi[u][1]});
            }
        }
    }
}

// Workgroups resident at once: the default grid of a sweep (every workgroup walks the same number of trips, so a second, partly
// filled round of workgroups would cost a whole round).  One figure per process: the devices of a cluster are of one kind.
template <typename R, bool PAIRED>
int resident_grid() {
    static const int grid = [] {
        int dev = 0, per_cu = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pauli_rot<R, PAIRED>, kTPB, 0) != hipSuccess || per_cu < 1)
            return 1024;
        return per_cu * prop.multiProcessorCount;
    }();
    return grid;
}

template <typename R, bool PAIRED>
hipError_t launch_prec(const LaunchCfg &cfg, void *a, void *b, const RotGeom &g, const RotSweep &sw) {
    RotTerms<R> rec{};
    for (int k = 0; k < sw.count; k++) {
        rec.z[k] = sw.z[k];
        rec.c[k] = (R)sw.c[k];
        rec.v[k] = (R)sw.v[k];
    }
    rec.odd = sw.odd_mask;
    rec.count = sw.count;
    constexpr uint64_t per_block = (uint64_t)kTPB * (PAIRED ? 4 : 8);
    uint64_t grid = (g.units + per_block - 1) / per_block;
    // QSIM_OPT_GRID_CAP > 0 caps the grid as it does for every kernel (a huge cap: one workgroup per block of units)
    const uint64_t cap = cfg.grid_cap > 0 ? (uint64_t)cfg.grid_cap : (uint64_t)resident_grid<R, PAIRED>();
    if (grid > cap) grid = cap;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL((k_pauli_rot<R, PAIRED>), dim3((unsigned)grid), dim3(kTPB), 0, cfg.stream, (R *)a, (R *)b, g, rec);
    return hipGetLastError();
}

} // namespace

hipError_t launch_pauli_rot(const LaunchCfg &cfg, void *a, void *b, bool f32, int n, const RotSweep &sw) {
    if (sw.count < 1 || sw.count > kMaxRotTermsPerSweep || n < 0 || n > 40 || !a || !b) return hipErrorInvalidValue;
    if (sw.full == (a == b)) return hipErrorInvalidValue; // every index counts exactly when the partner is another buffer
    const uint64_t N = 1ULL << n;
    if (sw.x >= N) return hipErrorInvalidValue; // the partner index must stay inside the buffer
    for (int k = 0; k < sw.count; k++)
        if (sw.z[k] >= N) return hipErrorInvalidValue;
    const bool paired = sw.x != 0 || sw.full;
    const int as = f32 ? 1 : 0; // log2 amplitudes per unit
    RotGeom g{};
    g.x = sw.x;
    g.amps = N;
    g.odd_slot = 1;
    g.low = ~0ULL;
    uint64_t amps_visited = N;
    if (sw.x != 0 && !sw.full) { // one member of each pair: the index with the highest bit of x clear
        const int h = 63 - __builtin_clzll(sw.x);
        amps_visited = N >> 1;
        if (h >= as) g.low = (1ULL << (h - as)) - 1ULL; // the zero is inserted at unit bit h - as
        else g.odd_slot = 0;                            // fp32, x == 1: both members share a unit; every unit, one pair each
    }
    g.units = g.odd_slot ? (amps_visited >> as) : N >> as;
    if (g.units == 0) g.units = 1; // one fp32 amplitude
    if (f32) return paired ? launch_prec<float, true>(cfg, a, b, g, sw) : launch_prec<float, false>(cfg, a, b, g, sw);
    return paired ? launch_prec<double, true>(cfg, a, b, g, sw) : launch_prec<double, false>(cfg, a, b, g, sw);
}

} // namespace qsim
