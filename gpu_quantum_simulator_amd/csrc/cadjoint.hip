// cadjoint.hip — the backward sweep of an adjoint gradient through CONTROLLED Pauli rotations (gfx950): k_pauli_adjoint's body walked
// with k_pauli_crot's geometry.  Its own object, like adjoint.hip and crot.hip, whose kernels stay as they are.  DESIGN §7f has the
// derivation; pauli_sweep.h has the geometry (CtrlGeom, ctrl_geom, spread), the term record and the device helpers.
//
// U_k = (1 - Pi_k) + Pi_k exp(-i theta_k/2 P_k), Pi_k = "every control qubit is 1", so dU_k/dtheta_k = -(i/2) Pi_k P_k U_k and
//     dE/dtheta_k = Im <lambda_k| Pi_k P_k |psi_k>:
// adjoint.hip's pair bracket summed over the pairs {j, j ^ x} INSIDE the control subspace only (controls and x | z are disjoint, so a
// visited index's partner has its controls set too), and U_k^+ changes psi and lambda only there.  A run of terms with one x and one
// control mask is differentiated and undone in registers, from its last term to its first, between one load and one store of the
// 2^-c of psi and of lambda that the subspace holds.
// From k_pauli_adjoint: the two buffers at the same indices, the fp64 accumulators, the unrolled term loop over expect_slots, the 2x2
// with the host's c and v of -theta, adjoint_units_per_trip, k_expect's reduction (no atomics) and reducing_grid.
// From k_pauli_crot: the insertion loop (spread), the uniform index parts kept per unit across a trip, the control bits OR-ed in, and
// the fp32 slot range — with a control on qubit 0 only the odd slot of a unit enters the sums and is rotated; the even slot of psi and
// of lambda is stored as it was loaded.  Every amplitude is written by exactly one thread: equal calls give equal bits.
#include "pauli_sweep.h"

namespace qsim {
namespace {

template <typename R, bool PAIRED, int KT>
__global__ __launch_bounds__(kTPB) void k_pauli_cadjoint(R *psi, R *lam, CtrlGeom g, RotTerms<R, KT> terms, double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2;       // amplitudes per unit
    constexpr int AS = A - 1;
    constexpr int U = adjoint_units_per_trip(PAIRED);
    static_assert((U & (U - 1)) == 0, "q0 is a multiple of U: E(q0 + u) = E(q0) | E(u)");
    const uint32_t tid = threadIdx.x;
    const bool two_units = PAIRED && g.odd_slot;    // the partner sits in a unit of its own (else: in the odd slot of a's unit)
    auto store = [&](R *p, uint64_t amp, const V &v) { *reinterpret_cast<V *>(p + 2 * amp) = v; };

    double acc[KT];
#pragma unroll
    for (int k = 0; k < KT; k++) acc[k] = 0.0;

    // the thread's own index bits, with the control bits (they meet no z): one parity bit per term, once
    const uint64_t jl = spread<R>(g, tid) | g.ones;
    uint32_t own = 0;
#pragma unroll
    for (int k = 0; k < KT; k++) own |= ((uint32_t)__builtin_popcountll(jl & terms.z[k]) & 1u) << k;
    const int first = A == 2 ? (int)g.first_slot : 0, slots = (A == 2 && g.odd_slot) ? 2 : 1;
    uint64_t eu[U];                                 // E(u << kTidBits): a trip's q0 is a multiple of U, so E(q0 + u) = E(q0) | E(u)
#pragma unroll
    for (int u = 0; u < U; u++) eu[u] = spread<R>(g, (uint64_t)u << kTidBits);

    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.units; q0 += (uint64_t)gridDim.x * U) {
        R ar[U][A], ai[U][A], br[U][A], bi[U][A];       // psi: the visited member and its partner
        R lar[U][A], lai[U][A], lbr[U][A], lbi[U][A];   // lambda, same indices
        const uint64_t j0 = spread<R>(g, q0 << kTidBits);
        uint64_t ju[U];                                 // uniform part of the amplitude index
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            ju[u] = j0 | eu[u];
            V va{}, vb{}, wa{}, wb{};
            if (t < g.units) {
                const uint64_t j = ju[u] | jl;
                va = load_unit(psi, j);
                wa = load_unit(lam, j);
                if (two_units) {
                    vb = load_unit(psi, (j ^ g.x) & ~(uint64_t)AS);
                    wb = load_unit(lam, (j ^ g.x) & ~(uint64_t)AS);
                }
            }
            if constexpr (A == 1) {
                ar[u][0] = va.x, ai[u][0] = va.y, br[u][0] = vb.x, bi[u][0] = vb.y;
                lar[u][0] = wa.x, lai[u][0] = wa.y, lbr[u][0] = wb.x, lbi[u][0] = wb.y;
            } else {
                ar[u][0] = va.x, ai[u][0] = va.y, ar[u][1] = va.z, ai[u][1] = va.w;
                lar[u][0] = wa.x, lai[u][0] = wa.y, lar[u][1] = wa.z, lai[u][1] = wa.w;
                if (PAIRED && !g.odd_slot) vb = V{va.z, va.w, 0.f, 0.f}, wb = V{wa.z, wa.w, 0.f, 0.f};            // x == 1: the pair is the unit
                else if (PAIRED && (g.x & 1)) vb = V{vb.z, vb.w, vb.x, vb.y}, wb = V{wb.z, wb.w, wb.x, wb.y};     // the partner sits in the other half of its unit
                br[u][0] = vb.x, bi[u][0] = vb.y, br[u][1] = vb.z, bi[u][1] = vb.w;
                lbr[u][0] = wb.x, lbi[u][0] = wb.y, lbr[u][1] = wb.z, lbi[u][1] = wb.w;
            }
        }
#pragma unroll
        for (int k = KT - 1; k >= 0; k--) { // unrolled: acc[k] stays a register; the guard and the term's record are uniform
            if (k >= terms.count) continue;
            const uint64_t z = terms.z[k];
            const R c = terms.c[k], v = terms.v[k];
            const bool odd = (terms.odd >> k) & 1u;
            const uint32_t mine = ((own >> k) & 1u) << 31;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t sg = parity_sign(ju[u], z) ^ mine;
#pragma unroll
                for (int s = 0; s < A; s++) {
                    if (s < first || s >= slots) continue; // a control on qubit 0: the even slot is outside the subspace
                    const uint32_t sgs = s ? odd_slot_sign(sg, z) : sg;
                    // every product of two floats is exact in fp64
                    const double pr = ar[u][s], pi = ai[u][s], mr = lar[u][s], mi = lai[u][s];
                    double t;
                    if (PAIRED) {
                        const double qr = br[u][s], qi = bi[u][s], nr = lbr[u][s], ni = lbi[u][s];
                        t = odd ? fma(nr, pr, ni * pi) - fma(mr, qr, mi * qi)       // Re [conj(lb) a - conj(la) b]
                                : fma(nr, pi, -(ni * pr)) + fma(mr, qi, -(mi * qr)); // Im [conj(lb) a + conj(la) b]
                    } else {
                        t = fma(mr, pi, -(mi * pr));                                 // Im conj(la) a
                    }
                    acc[k] += flip(t, sgs);
                    const R sv = flip(v, sgs);
                    if (PAIRED) {
                        rotate_pair(ar[u][s], ai[u][s], br[u][s], bi[u][s], c, sv, odd);
                        rotate_pair(lar[u][s], lai[u][s], lbr[u][s], lbi[u][s], c, sv, odd);
                    } else {
                        rotate_diag(ar[u][s], ai[u][s], c, sv);
                        rotate_diag(lar[u][s], lai[u][s], c, sv);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            if (t >= g.units) continue;
            const uint64_t j = ju[u] | jl, p = (j ^ g.x) & ~(uint64_t)AS;
            const bool same = PAIRED && !g.odd_slot, swapped = (g.x & 1) != 0;
            store(psi, j, own_unit(same, ar[u], ai[u], br[u], bi[u]));
            store(lam, j, own_unit(same, lar[u], lai[u], lbr[u], lbi[u]));
            if (two_units) {
                store(psi, p, partner_unit(swapped, br[u], bi[u]));
                store(lam, p, partner_unit(swapped, lbr[u], lbi[u]));
            }
        }
    }

    // k_expect's reduction; the thread's own parity is already in the sums
    __shared__ double part[kTPB / 64][KT];
#pragma unroll
    for (int k = 0; k < KT; k++) {
        double v = acc[k];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if ((tid & 63) == 0) part[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < KT) {
        double s = 0.0;
        for (int w = 0; w < kTPB / 64; w++) s += part[w][tid];
        partial[(uint64_t)blockIdx.x * KT + tid] = s;
    }
}

template <typename R, bool PAIRED, int KT>
hipError_t launch_kt(hipStream_t stream, void *psi, void *lam, const CtrlGeom &g, const RotSweep &sw, double *d_partial, double *d_out) {
    RotTerms<R, KT> rec{};
    fill_terms(rec, sw);
    const unsigned grid = reducing_grid<k_pauli_cadjoint<R, PAIRED, KT>>(g.units, (uint64_t)kTPB * adjoint_units_per_trip(PAIRED));
    hipLaunchKernelGGL((k_pauli_cadjoint<R, PAIRED, KT>), dim3(grid), dim3(kTPB), 0, stream, (R *)psi, (R *)lam, g, rec, d_partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_expect_final(stream, d_partial, (int)grid, KT, d_out);
}

} // namespace

hipError_t launch_pauli_cadjoint(const LaunchCfg &cfg, void *psi, void *lam, bool f32, int n, uint64_t controls, const RotSweep &sw, double *d_partial,
                                 double *d_out) {
    if (!check_sweep(sw, n) || sw.full || n < 1 || !psi || !lam || psi == lam || !d_partial || !d_out) return hipErrorInvalidValue;
    if (controls == 0 || controls >= (1ULL << n) || (controls & sw.x)) return hipErrorInvalidValue;
    for (int k = 0; k < sw.count; k++)
        if (sw.z[k] & controls) return hipErrorInvalidValue; // a sign of the sum as well as of v: refused, not folded
    const CtrlGeom g = ctrl_geom(controls, sw.x, f32, n);
    return for_precision_and_pairing(f32, sw.x != 0, [&](auto r, auto p) {
        return for_term_slots(sw.count, [&](auto kt) {
            return launch_kt<decltype(r), decltype(p)::value, decltype(kt)::value>(cfg.stream, psi, lam, g, sw, d_partial, d_out);
        });
    });
}

} // namespace qsim
