// evolve.hip — Pauli-string rotations exp(-i theta/2 P) as in-place sweeps (gfx950).  Its own object, like expect.hip: nothing
// here is compiled into kernels.hip, whose code layout is part of the measured product.  pauli_sweep.h says how a
// sweep walks a state (units, bit insertion, parity split, fp32 corners, grids) and has the term record, the 2x2 itself (rotate_pair,
// rotate_diag) and the packing for the stores, which the adjoint sweep uses too; this file has the rule and the kernel.
//
// P maps every index pair {j, j ^ x} to itself, so the rotation is a 2x2 on each pair whatever the string's weight.  With
// s(j) = (-1)^popcount(j & z), ny = popcount(x & z), c = cos(theta/2) and w = -i sin(theta/2) i^ny:
//     a_j'       = c a_j       + w (-1)^ny s(j) b_(j^x)
//     b_(j^x)'   = c b_(j^x)   + w s(j) a_j
// w is real for odd ny and imaginary for even ny, so the host hands over c and ONE real number v per term (w = v or w = i v) and
// a bit that says which; the device selects signs and never sees an angle.  x == 0 is the diagonal case of the same rule
// (b = a, ny = 0): a_j' = (c + i v s(j)) a_j with v = -sin(theta/2).
// Consecutive terms that share x map the same pairs to themselves: a run of up to kMaxPauliTermsPerSweep of them is applied in
// registers, in the caller's order, between one load and one store of the state.  The thread's own part of popcount(j & z) is one
// bit per term, formed once before the loop.  Every amplitude is written by exactly one thread: no atomics, no reduction, equal
// calls give equal bits.
#include "pauli_sweep.h"

namespace qsim {
namespace {

constexpr int KT = kMaxPauliTermsPerSweep;

template <typename R, bool PAIRED>
__global__ __launch_bounds__(kTPB) void k_pauli_rot(R *a, R *b, SweepGeom g, RotTerms<R, KT> terms) { // a and b may be one buffer
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2;       // amplitudes per unit
    constexpr int AS = A - 1;
    constexpr int U = units_per_trip(PAIRED);
    const uint32_t tid = threadIdx.x;
    const bool two_units = PAIRED && g.odd_slot;    // the partner sits in a unit of its own (else: in the odd slot of a's unit)
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
    const uint64_t jl = expand<R>(g, tid);
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
                const uint64_t j = expand<R>(g, t);
                va = load_unit(a, j);
                if (two_units) vb = load_unit(b, (j ^ g.x) & ~(uint64_t)AS);
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
                const uint64_t ju = expand<R>(g, (q0 + u) << kTidBits); // uniform part of the amplitude index
                const uint32_t sg = parity_sign(ju, z) ^ mine;
#pragma unroll
                for (int s = 0; s < A; s++) {
                    if (s >= slots) continue;
                    const R sv = flip(v, s ? odd_slot_sign(sg, z) : sg);
                    if (PAIRED) rotate_pair(ar[u][s], ai[u][s], br[u][s], bi[u][s], c, sv, odd);
                    else rotate_diag(ar[u][s], ai[u][s], c, sv);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            if (t >= g.units) continue;
            const uint64_t j = expand<R>(g, t);
            store(a, j, own_unit(PAIRED && !g.odd_slot, ar[u], ai[u], br[u], bi[u]));
            if (two_units) store(b, (j ^ g.x) & ~(uint64_t)AS, partner_unit((g.x & 1) != 0, br[u], bi[u]));
        }
    }
}

template <typename R, bool PAIRED>
hipError_t launch_prec(const LaunchCfg &cfg, void *a, void *b, const SweepGeom &g, const RotSweep &sw) {
    RotTerms<R, KT> rec{};
    fill_terms(rec, sw);
    const unsigned grid = writing_grid<k_pauli_rot<R, PAIRED>>(cfg, g.units, (uint64_t)kTPB * units_per_trip(PAIRED));
    hipLaunchKernelGGL((k_pauli_rot<R, PAIRED>), dim3(grid), dim3(kTPB), 0, cfg.stream, (R *)a, (R *)b, g, rec);
    return hipGetLastError();
}

} // namespace

hipError_t launch_pauli_rot(const LaunchCfg &cfg, void *a, void *b, bool f32, int n, const RotSweep &sw) {
    if (!check_sweep(sw, n) || !a || !b) return hipErrorInvalidValue;
    if (sw.full == (a == b)) return hipErrorInvalidValue; // every index counts exactly when the partner is another buffer
    const bool paired = sw.x != 0 || sw.full;
    const SweepGeom g = sweep_geom(sw.x, sw.full, f32, n);
    return for_precision_and_pairing(f32, paired, [&](auto r, auto p) { return launch_prec<decltype(r), decltype(p)::value>(cfg, a, b, g, sw); });
}

} // namespace qsim
