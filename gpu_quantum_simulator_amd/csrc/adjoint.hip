// adjoint.hip — adjoint-mode gradients of <H> for circuits of Pauli rotations (gfx950): the fused backward sweep k_pauli_adjoint and
// the out-of-place lambda = H psi, k_pauli_sum.  Its own object, like expect.hip and evolve.hip: nothing here is compiled into
// kernels.hip.  pauli_sweep.h says how a sweep walks a state (units, bit insertion, parity split, fp32 corners, grids) and has the term
// record and the device helpers the sweeps share; DESIGN §7d has the derivation.
//
// Backward sweep.  With |lambda_k> = U_(k+1)^+ ... U_K^+ H |psi_K>, dE/dtheta_k = Im <lambda_k|P_k|psi_k>, and with a = psi_j,
// b = psi_(j^x), la = lambda_j, lb = lambda_(j^x), s(j) = (-1)^popcount(j & z), ny = popcount(x & z):
//     <lambda|P|psi> = i^ny sum_pairs s(j) [conj(lb) a + (-1)^ny conj(la) b]          (x == 0: sum_j s(j) conj(la) a)
// Every term of one x maps the same pairs to themselves, so a run of terms is differentiated AND undone in registers, from its last
// term to its first, between one load and one store of psi and lambda: term k adds s(j) times the real (odd ny) or imaginary (even
// ny) part of the bracket to its fp64 accumulator and then applies U_k^+ — k_pauli_rot's 2x2 with the host's c and v of -theta_k —
// to (a, b) and to (la, lb).  i^ny and the choice of sign are the host's.  The reduction is k_expect's: wave butterfly, waves added
// in order through LDS, one row per workgroup, launch_expect_final; no atomics, equal calls give equal bits.
//
// lambda = H psi.  For one x and output index i:  dst_i (=|+=) psi_(i^x) sum_t c_t i^(ny_t) s_t(i^x).  A gather: a thread owns its
// output units and reads the partner units, which permute the same 128-byte lines.  s_t(i^x) = (-1)^ny_t s_t(i), so the host folds
// that sign and the non-zero component of i^ny_t into one real number per term and a bit that says whether it is the real or the
// imaginary part of the weight.
#include "pauli_sweep.h"

namespace qsim {
namespace {

template <typename R, bool PAIRED, int KT>
__global__ __launch_bounds__(kTPB) void k_pauli_adjoint(R *psi, R *lam, SweepGeom g, RotTerms<R, KT> terms, double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2;       // amplitudes per unit
    constexpr int AS = A - 1;
    constexpr int U = adjoint_units_per_trip(PAIRED);
    const uint32_t tid = threadIdx.x;
    const bool two_units = PAIRED && g.odd_slot;    // the partner sits in a unit of its own (else: in the odd slot of a's unit)
    auto store = [&](R *p, uint64_t amp, const V &v) {
        if constexpr (A == 2) if (g.amps < 2) {
            *reinterpret_cast<float2 *>(p) = float2{v.x, v.y};
            return;
        }
        *reinterpret_cast<V *>(p + 2 * amp) = v;
    };

    double acc[KT];
#pragma unroll
    for (int k = 0; k < KT; k++) acc[k] = 0.0;

    // the thread's own index bits: one parity bit per term, once
    const uint64_t jl = expand<R>(g, tid);
    uint32_t own = 0;
#pragma unroll
    for (int k = 0; k < KT; k++) own |= ((uint32_t)__builtin_popcountll(jl & terms.z[k]) & 1u) << k;
    const int slots = (A == 2 && g.odd_slot) ? 2 : 1;

    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.units; q0 += (uint64_t)gridDim.x * U) {
        R ar[U][A], ai[U][A], br[U][A], bi[U][A];       // psi: the visited member and its partner
        R lar[U][A], lai[U][A], lbr[U][A], lbi[U][A];   // lambda, same indices
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            V va{}, vb{}, wa{}, wb{};
            if (t < g.units) {
                const uint64_t j = expand<R>(g, t);
                va = load_unit_or_one(g, psi, j);
                wa = load_unit_or_one(g, lam, j);
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
                const uint64_t ju = expand<R>(g, (q0 + u) << kTidBits); // uniform part of the amplitude index
                const uint32_t sg = parity_sign(ju, z) ^ mine;
#pragma unroll
                for (int s = 0; s < A; s++) {
                    if (s >= slots) continue;
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
            const uint64_t j = expand<R>(g, t), p = (j ^ g.x) & ~(uint64_t)AS;
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
hipError_t launch_kt(hipStream_t stream, void *psi, void *lam, const SweepGeom &g, const RotSweep &sw, double *d_partial, double *d_out) {
    RotTerms<R, KT> rec{};
    fill_terms(rec, sw);
    const unsigned grid = reducing_grid<k_pauli_adjoint<R, PAIRED, KT>>(g.units, (uint64_t)kTPB * adjoint_units_per_trip(PAIRED));
    hipLaunchKernelGGL((k_pauli_adjoint<R, PAIRED, KT>), dim3(grid), dim3(kTPB), 0, stream, (R *)psi, (R *)lam, g, rec, d_partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_expect_final(stream, d_partial, (int)grid, KT, d_out);
}

// ---- lambda = H psi ---------------------------------------------------------------------------------------------------------------
constexpr int KS = kMaxPauliTermsPerSweep;
constexpr int kSumUnits = 4; // units per thread and trip: 4 loads of the source in flight, and 4 of the destination when it accumulates

template <typename R>
struct SumTerms {       // by value: scalar loads
    uint64_t z[KS];
    R c[KS];            // c_t times the non-zero component of i^ny times (-1)^ny, rounded once to the state's precision by the host
    uint32_t odd;       // bit k: ny is odd — the term adds to the imaginary part of the weight; else to the real part
    int32_t count;
};

// g: the geometry of x == 0 (every unit, nothing inserted) with g.x = the group's x
template <typename R>
__global__ __launch_bounds__(kTPB) void k_pauli_sum(const R *__restrict__ src, R *__restrict__ dst, SweepGeom g, SumTerms<R> terms, int accumulate) {
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2;
    constexpr int AS = A - 1;
    constexpr int U = kSumUnits;
    const uint32_t tid = threadIdx.x;
    const bool tiny = A == 2 && g.amps < 2; // a register of one fp32 amplitude is 8 bytes long

    const uint64_t il = expand<R>(g, tid);
    uint32_t own = 0;
    for (int k = 0; k < terms.count; k++) own |= ((uint32_t)__builtin_popcountll(il & terms.z[k]) & 1u) << k;

    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.units; q0 += (uint64_t)gridDim.x * U) {
        V vs[U], vd[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            vs[u] = V{};
            vd[u] = V{};
            if (t < g.units) {
                const uint64_t i = expand<R>(g, t);
                vs[u] = load_unit_or_one(g, src, (i ^ g.x) & ~(uint64_t)AS);
                if (accumulate) vd[u] = load_unit_or_one(g, dst, i);
            }
        }
        R wr[U][A], wi[U][A]; // the weight of output slot s of unit u
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int s = 0; s < A; s++) wr[u][s] = wi[u][s] = (R)0;
        for (int k = 0; k < terms.count; k++) { // uniform: the term's record comes through scalar loads
            const uint64_t z = terms.z[k];
            const R c = terms.c[k];
            const bool odd = (terms.odd >> k) & 1u;
            const uint32_t mine = ((own >> k) & 1u) << 31;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t iu = expand<R>(g, (q0 + u) << kTidBits); // uniform part of the output index
                const uint32_t sg = parity_sign(iu, z) ^ mine;
#pragma unroll
                for (int s = 0; s < A; s++) {
                    const R f = flip(c, s ? odd_slot_sign(sg, z) : sg);
                    if (odd) wi[u][s] += f;
                    else wr[u][s] += f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            if (t >= g.units) continue;
            const uint64_t i = expand<R>(g, t);
            V out;
            if constexpr (A == 1) {
                out = V{fma(-wi[u][0], vs[u].y, wr[u][0] * vs[u].x) + vd[u].x, fma(wi[u][0], vs[u].x, wr[u][0] * vs[u].y) + vd[u].y};
                *reinterpret_cast<V *>(dst + 2 * i) = out;
            } else {
                V p = vs[u];
                if (g.x & 1) p = V{p.z, p.w, p.x, p.y}; // the partner sits in the other half of its unit
                out = V{fma(-wi[u][0], p.y, wr[u][0] * p.x) + vd[u].x, fma(wi[u][0], p.x, wr[u][0] * p.y) + vd[u].y,
                        fma(-wi[u][1], p.w, wr[u][1] * p.z) + vd[u].z, fma(wi[u][1], p.z, wr[u][1] * p.w) + vd[u].w};
                if (tiny) *reinterpret_cast<float2 *>(dst) = float2{out.x, out.y};
                else *reinterpret_cast<V *>(dst + 2 * i) = out;
            }
        }
    }
}

template <typename R>
hipError_t launch_sum_prec(const LaunchCfg &cfg, const void *src, void *dst, const SweepGeom &g, const SumSweep &sw) {
    SumTerms<R> rec{};
    fill_terms(rec, sw);
    const unsigned grid = writing_grid<k_pauli_sum<R>>(cfg, g.units, (uint64_t)kTPB * kSumUnits);
    hipLaunchKernelGGL((k_pauli_sum<R>), dim3(grid), dim3(kTPB), 0, cfg.stream, (const R *)src, (R *)dst, g, rec, sw.accumulate ? 1 : 0);
    return hipGetLastError();
}

} // namespace

hipError_t launch_pauli_adjoint(const LaunchCfg &cfg, void *psi, void *lam, bool f32, int n, const RotSweep &sw, double *d_partial, double *d_out) {
    if (!check_sweep(sw, n) || sw.full || !psi || !lam || psi == lam || !d_partial || !d_out) return hipErrorInvalidValue;
    const bool paired = sw.x != 0;
    const SweepGeom g = sweep_geom(sw.x, false, f32, n);
    return for_precision_and_pairing(f32, paired, [&](auto r, auto p) {
        return for_term_slots(sw.count, [&](auto kt) {
            return launch_kt<decltype(r), decltype(p)::value, decltype(kt)::value>(cfg.stream, psi, lam, g, sw, d_partial, d_out);
        });
    });
}

hipError_t launch_pauli_sum(const LaunchCfg &cfg, const void *src, void *dst, bool f32, int n, const SumSweep &sw) {
    if (!check_sweep(sw, n) || sw.full || !src || !dst || src == dst) return hipErrorInvalidValue;
    SweepGeom g = sweep_geom(0, false, f32, n); // every output unit
    g.x = sw.x;
    return f32 ? launch_sum_prec<float>(cfg, src, dst, g, sw) : launch_sum_prec<double>(cfg, src, dst, g, sw);
}

} // namespace qsim
