// expect.hip — Pauli-string expectation values <psi|P|psi> as read-only reduction sweeps (gfx950).  Its own object: nothing here
// is compiled into kernels.hip, whose code layout is part of the measured product.  pauli_sweep.h says how a sweep
// walks a state (units, bit insertion, parity split, fp32 corners, grids); this file has what the reduction adds.
//
// With s(j) = (-1)^popcount(j & z):
//   x == 0:  <P> = sum_j s(j) |psi_j|^2
//   x != 0:  h = highest bit of x; over the j with bit h clear, c = conj(psi_(j^x)) psi_j:
//            <P> = +-2 sum_j s(j) Re c  (popcount(x & z) even)   or   +-2 sum_j s(j) Im c  (odd)
// All strings of one x share the loads and c; a term costs a parity, a select and an add.  The kernel forms the plain
// signed sums; the constant factor (+-1, +-2) is the host's.  The thread's own part of popcount(j & z) is applied ONCE, to the
// thread's finished sums.
//
// Reduction, no atomics: fp64 sums per thread -> xor butterfly in the wave -> waves added in order through LDS -> one row of
// partial sums per workgroup -> k_expect_final adds the rows in a fixed order (launch_expect_final: the adjoint sweep ends the same
// way).  Same bits from call to call.
#include "pauli_sweep.h"

namespace qsim {
namespace {

template <int KT>
struct TermRec {        // by value: scalar loads
    uint64_t z[KT];     // unused slots: 0
    uint32_t im;        // bit k: term k sums Im c instead of Re c (paired sweeps)
};

template <typename R, bool PAIRED, int KT>
__global__ __launch_bounds__(kTPB) void k_expect(const R *__restrict__ a, const R *__restrict__ b, SweepGeom g, TermRec<KT> terms,
                                                 double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2;       // amplitudes per unit
    constexpr int AS = A - 1;
    constexpr int U = units_per_trip(PAIRED);
    const uint32_t tid = threadIdx.x;

    double acc[KT];
#pragma unroll
    for (int k = 0; k < KT; k++) acc[k] = 0.0;

    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.units; q0 += (uint64_t)gridDim.x * U) {
        V va[U], vb[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            va[u] = V{};
            vb[u] = V{};
            if (t < g.units) {
                const uint64_t j = expand<R>(g, t);
                va[u] = load_unit_or_one(g, a, j);
                if (PAIRED) vb[u] = load_unit_or_one(g, b, (j ^ g.x) & ~(uint64_t)AS);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t ju = expand<R>(g, (q0 + u) << kTidBits); // uniform part of the amplitude index
            double re[A], im[A] = {};                         // per slot: Re c, Im c — or |psi|^2 in re
            if constexpr (A == 1) {
                const double ar = va[u].x, ai = va[u].y;
                if (PAIRED) {
                    const double br = vb[u].x, bi = vb[u].y;
                    re[0] = fma(ar, br, ai * bi);
                    im[0] = fma(ai, br, -(ar * bi));
                } else {
                    re[0] = fma(ar, ar, ai * ai);
                }
            } else {
                // every product of two floats is exact in fp64
                const float4 fa = *reinterpret_cast<const float4 *>(&va[u]);
                float4 fb = *reinterpret_cast<const float4 *>(&vb[u]);
                if (PAIRED && (g.x & 1)) fb = float4{fb.z, fb.w, fb.x, fb.y}; // the partner sits in the other half of its unit
                const double ar[2] = {(double)fa.x, g.odd_slot ? (double)fa.z : 0.0}, ai[2] = {(double)fa.y, g.odd_slot ? (double)fa.w : 0.0};
                const double br[2] = {(double)fb.x, (double)fb.z}, bi[2] = {(double)fb.y, (double)fb.w};
#pragma unroll
                for (int s = 0; s < A; s++) {
                    if (PAIRED) {
                        re[s] = fma(ar[s], br[s], ai[s] * bi[s]);
                        im[s] = fma(ai[s], br[s], -(ar[s] * bi[s]));
                    } else {
                        re[s] = fma(ar[s], ar[s], ai[s] * ai[s]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < KT; k++) {
                const uint64_t z = terms.z[k];
                const uint32_t sg = parity_sign(ju, z); // scalar
                const bool use_im = PAIRED && ((terms.im >> k) & 1u);
#pragma unroll
                for (int s = 0; s < A; s++) {
                    const double v = use_im ? im[s] : re[s];
                    acc[k] += flip(v, s ? odd_slot_sign(sg, z) : sg);
                }
            }
        }
    }

    // the thread's own index bits, once
    const uint64_t jl = expand<R>(g, tid);
    __shared__ double part[kTPB / 64][KT];
#pragma unroll
    for (int k = 0; k < KT; k++) {
        double v = flip(acc[k], parity_sign(jl, terms.z[k]));
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
hipError_t launch_kt(hipStream_t stream, const void *a, const void *b, const SweepGeom &g, const ExpectSweep &sw, double *d_partial,
                     double *d_out) {
    TermRec<KT> rec{};
    for (int k = 0; k < sw.count && k < KT; k++) rec.z[k] = sw.z[k];
    rec.im = sw.im_mask;
    const unsigned grid = reducing_grid<k_expect<R, PAIRED, KT>>(g.units, (uint64_t)kTPB * units_per_trip(PAIRED));
    hipLaunchKernelGGL((k_expect<R, PAIRED, KT>), dim3(grid), dim3(kTPB), 0, stream, (const R *)a, (const R *)b, g, rec, d_partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_expect_final(stream, d_partial, (int)grid, KT, d_out);
}

} // namespace

// out[k] = sum over the rows of `partial` in a fixed order: lane l adds rows l, l + 64, ... in order, then the butterfly.
static __global__ __launch_bounds__(64) void k_expect_final(const double *__restrict__ partial, int rows, int kt, double *__restrict__ out) {
    const int k = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < rows; r += 64) s += partial[(size_t)r * kt + k];
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (threadIdx.x == 0) out[k] = s;
}

hipError_t launch_expect_final(hipStream_t stream, const double *d_partial, int rows, int kt, double *d_out) {
    hipLaunchKernelGGL(k_expect_final, dim3(kt), dim3(64), 0, stream, d_partial, rows, kt, d_out);
    return hipGetLastError();
}

int expect_slots(int count) { return count <= 1 ? 1 : count <= 8 ? 8 : count <= 16 ? 16 : count <= kMaxPauliTermsPerSweep ? 32 : 0; }

hipError_t launch_expect(const LaunchCfg &cfg, const void *a, const void *b, bool f32, int n, const ExpectSweep &sw, double *d_partial,
                         double *d_out) {
    if (!check_sweep(sw, n)) return hipErrorInvalidValue;
    const bool paired = sw.x != 0 || sw.full;
    const SweepGeom g = sweep_geom(sw.x, sw.full, f32, n);
    return for_precision_and_pairing(f32, paired, [&](auto r, auto p) {
        return for_term_slots(sw.count, [&](auto kt) {
            return launch_kt<decltype(r), decltype(p)::value, decltype(kt)::value>(cfg.stream, a, b, g, sw, d_partial, d_out);
        });
    });
}

} // namespace qsim
