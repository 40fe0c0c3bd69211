// crot.hip — controlled Pauli-string rotations [(1 - Pi) + Pi exp(-i theta/2 P)], Pi = "every control qubit is 1", as in-place
// sweeps of the control subspace alone (gfx950).  Its own object, like evolve.hip, whose kernel it is the sibling of: the same
// pairs {j, j ^ x}, the same 2x2 (rotate_pair, rotate_diag), the same term records with c and v as the host forms them for an
// uncontrolled term — applied only where (j & controls) == controls.  Controls and x | z are disjoint, so the partner j ^ x of a
// visited index has its controls set too, and the pair rule of evolve.hip holds unchanged on the 2^(n-c) indices of the subspace.
//
// pauli_sweep.h has the geometry (CtrlGeom, ctrl_geom): a unit index becomes an amplitude index by inserting a zero at h, the
// highest bit of x, and at every control position, lowest first, and OR-ing the control bits in.  Inserting zeros is linear over
// OR, so the parity split of the other sweeps stays: E(q << kTidBits) is uniform over the workgroup (scalar unit: one expansion per
// trip, OR-ed with the U expansions of u << kTidBits formed before the loop), E(tid) is the thread's own and formed once; the
// control bits carry no z (the host folds a z bit there into v).
// A sweep with c controls visits 2^-c of the units of the uncontrolled sweep of the same x.  fp64: a control below bit 3 thins the
// 128-byte lines, it does not break them up.  fp32: a control on qubit 0 leaves the odd slot of every visited unit as the only
// active one; the unit — and its partner unit — is loaded, rotated in that slot and stored whole, the thread owns both.
// Every amplitude is written by exactly one thread: no atomics, equal calls give equal bits, and an amplitude inside the subspace
// gets the bits k_pauli_rot gives it.
#include "pauli_sweep.h"

namespace qsim {
namespace {

constexpr int KT = kMaxPauliTermsPerSweep;

template <typename R, bool PAIRED>
__global__ __launch_bounds__(kTPB) void k_pauli_crot(R *a, CtrlGeom g, RotTerms<R, KT> terms) {
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2;       // amplitudes per unit
    constexpr int AS = A - 1;
    constexpr int U = units_per_trip(PAIRED);       // the loads in flight of k_pauli_rot
    static_assert((U & (U - 1)) == 0, "q0 is a multiple of U: E(q0 + u) = E(q0) | E(u)");
    const uint32_t tid = threadIdx.x;
    const bool two_units = PAIRED && g.odd_slot;    // the partner sits in a unit of its own (else: in the odd slot of a's unit)
    auto store = [&](uint64_t amp, const V &v) { *reinterpret_cast<V *>(a + 2 * amp) = v; };

    // the thread's own index bits, with the control bits (they meet no z): one parity bit per term, once
    const uint64_t jl = spread<R>(g, tid) | g.ones;
    uint32_t own = 0;
    for (int k = 0; k < terms.count; k++) own |= ((uint32_t)__builtin_popcountll(jl & terms.z[k]) & 1u) << k;
    const int first = A == 2 ? (int)g.first_slot : 0, slots = (A == 2 && g.odd_slot) ? 2 : 1;
    uint64_t eu[U];                                 // E(u << kTidBits): a trip's q0 is a multiple of U, so E(q0 + u) = E(q0) | E(u)
#pragma unroll
    for (int u = 0; u < U; u++) eu[u] = spread<R>(g, (uint64_t)u << kTidBits);

    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.units; q0 += (uint64_t)gridDim.x * U) {
        R ar[U][A], ai[U][A], br[U][A], bi[U][A];
        const uint64_t j0 = spread<R>(g, q0 << kTidBits);
        uint64_t ju[U];                             // uniform part of the amplitude index
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            ju[u] = j0 | eu[u];
            V va{}, vb{};
            if (t < g.units) {
                const uint64_t j = ju[u] | jl;
                va = load_unit(a, j);
                if (two_units) vb = load_unit(a, (j ^ g.x) & ~(uint64_t)AS);
            }
            if constexpr (A == 1) {
                ar[u][0] = va.x, ai[u][0] = va.y;
                br[u][0] = vb.x, bi[u][0] = vb.y;
            } else {
                ar[u][0] = va.x, ai[u][0] = va.y, ar[u][1] = va.z, ai[u][1] = va.w;
                if (PAIRED && !g.odd_slot) vb = V{va.z, va.w, 0.f, 0.f};                   // x == 1: the pair is the unit
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
                const uint32_t sg = parity_sign(ju[u], z) ^ mine;
#pragma unroll
                for (int s = 0; s < A; s++) {
                    if (s < first || s >= slots) continue;
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
            const uint64_t j = ju[u] | jl;
            store(j, own_unit(PAIRED && !g.odd_slot, ar[u], ai[u], br[u], bi[u]));
            if (two_units) store((j ^ g.x) & ~(uint64_t)AS, partner_unit((g.x & 1) != 0, br[u], bi[u]));
        }
    }
}

template <typename R, bool PAIRED>
hipError_t launch_prec(const LaunchCfg &cfg, void *a, const CtrlGeom &g, const RotSweep &sw) {
    RotTerms<R, KT> rec{};
    fill_terms(rec, sw);
    const unsigned grid = writing_grid<k_pauli_crot<R, PAIRED>>(cfg, g.units, (uint64_t)kTPB * units_per_trip(PAIRED));
    hipLaunchKernelGGL((k_pauli_crot<R, PAIRED>), dim3(grid), dim3(kTPB), 0, cfg.stream, (R *)a, g, rec);
    return hipGetLastError();
}

} // namespace

hipError_t launch_pauli_crot(const LaunchCfg &cfg, void *a, bool f32, int n, uint64_t controls, const RotSweep &sw) {
    if (!check_sweep(sw, n) || !a || sw.full || n < 1) return hipErrorInvalidValue;
    if (controls == 0 || controls >= (1ULL << n) || (controls & sw.x)) return hipErrorInvalidValue;
    RotSweep in = sw; // on a control qubit Z is the constant -1: a sign of the term, not an index bit of the sweep
    for (int k = 0; k < in.count; k++) {
        if (__builtin_popcountll(in.z[k] & controls) & 1) in.v[k] = -in.v[k];
        in.z[k] &= ~controls;
    }
    const CtrlGeom g = ctrl_geom(controls, sw.x, f32, n);
    return for_precision_and_pairing(f32, sw.x != 0, [&](auto r, auto p) { return launch_prec<decltype(r), decltype(p)::value>(cfg, a, g, in); });
}

} // namespace qsim
