// expect.hip — Pauli-string expectation values <psi|P|psi> as read-only reduction sweeps (gfx950).  Its own object: nothing here
// is compiled into kernels.hip, whose code layout is part of the measured product.
//
// A string is two masks: x (bit q: X or Y on qubit q) and z (bit q: Z or Y).  With s(j) = (-1)^popcount(j & z):
//   x == 0:  <P> = sum_j s(j) |psi_j|^2
//   x != 0:  h = highest bit of x; over the j with bit h clear, c = conj(psi_(j^x)) psi_j:
//            <P> = +-2 sum_j s(j) Re c  (popcount(x & z) even)   or   +-2 sum_j s(j) Im c  (odd)
// All strings of one x share the loads and c; a term costs a parity, a select and an add.  The kernel forms the plain
// signed sums; the constant factor (+-1, +-2) is the host's.
//
// Work is dealt in UNITS of 16 bytes per lane (one fp64 amplitude, two fp32 amplitudes), consecutive lanes on consecutive
// units; the partner unit (j ^ x) permutes the same 128-byte lines, so both streams stay coalesced for any x.  A unit index
// t = (q << 8) | tid is expanded to an amplitude index by a bit insertion (the zero at bit h), which is linear over OR of
// disjoint bit sets: popcount(j & z) = popcount(E(q << 8) & z) + popcount(E(tid) & z) (+ z bit 0 for the odd fp32 slot).
// The first part is uniform over the workgroup (scalar unit), the second is constant per thread and is applied ONCE, to
// the thread's finished sums.
//
// Reduction, no atomics: fp64 sums per thread -> xor butterfly in the wave -> waves added in order through LDS -> one row of
// partial sums per workgroup -> k_expect_final adds the rows in a fixed order.  Same bits from call to call.
#include "qsim_internal.h"

namespace qsim {
namespace {

constexpr int kTPB = 256;                     // 4 waves; a unit index's low 8 bits are the thread
constexpr int kTidBits = 8;
static_assert((1 << kTidBits) == kTPB, "unit index = (q << kTidBits) | tid");

template <int KT>
struct TermRec {        // by value: scalar loads
    uint64_t z[KT];     // unused slots: 0
    uint32_t im;        // bit k: term k sums Im c instead of Re c (paired sweeps)
};

struct SweepGeom {
    uint64_t units;     // 16-byte units to visit
    uint64_t low;       // unit-index bits below the inserted zero (all ones: nothing inserted)
    uint64_t x;         // partner amplitude = amplitude ^ x
    uint64_t amps;      // amplitudes in the buffer (guards the one-amplitude fp32 register)
    uint32_t odd_slot;  // fp32: the odd amplitude of a unit counts too (0 only for x == 1 on one state: j runs over even indices)
};

template <typename R> struct Vec16;
template <> struct Vec16<double> { using type = double2; };
template <> struct Vec16<float> { using type = float4; };

__device__ __forceinline__ double flip(double v, uint32_t sign_bit31) {
    return __hiloint2double(__double2hiint(v) ^ (int)sign_bit31, __double2loint(v));
}

template <typename R, bool PAIRED, int KT>
__global__ __launch_bounds__(kTPB) void k_expect(const R *__restrict__ a, const R *__restrict__ b, SweepGeom g, TermRec<KT> terms,
                                                 double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2;       // amplitudes per unit
    constexpr int AS = A - 1;
    constexpr int U = PAIRED ? 4 : 8;               // units per thread and trip: 8 independent 16-byte loads in flight
    const uint32_t tid = threadIdx.x;
    auto expand = [&](uint64_t t) { return (((t & ~g.low) << 1) | (t & g.low)) << AS; }; // unit index -> its (even) amplitude index
    auto load = [&](const R *p, uint64_t amp) -> V {
        if constexpr (A == 2) if (g.amps < 2) { // a register of one fp32 amplitude is 8 bytes long
            const float2 one = *reinterpret_cast<const float2 *>(p);
            V v{};
            v.x = one.x;
            v.y = one.y;
            return v;
        }
        return *reinterpret_cast<const V *>(p + 2 * amp);
    };

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
                const uint64_t j = expand(t);
                va[u] = load(a, j);
                if (PAIRED) vb[u] = load(b, (j ^ g.x) & ~(uint64_t)AS);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t ju = expand((q0 + u) << kTidBits); // uniform part of the amplitude index
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
                const uint32_t sg = ((uint32_t)__builtin_popcountll(ju & z) & 1u) << 31; // scalar
                const bool use_im = PAIRED && ((terms.im >> k) & 1u);
#pragma unroll
                for (int s = 0; s < A; s++) {
                    const double v = use_im ? im[s] : re[s];
                    acc[k] += flip(v, s ? sg ^ ((uint32_t)(z & 1ULL) << 31) : sg);
                }
            }
        }
    }

    // the thread's own index bits, once
    const uint64_t jl = expand(tid);
    __shared__ double part[kTPB / 64][KT];
#pragma unroll
    for (int k = 0; k < KT; k++) {
        double v = flip(acc[k], ((uint32_t)__builtin_popcountll(jl & terms.z[k]) & 1u) << 31);
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

// out[k] = sum over the rows of `partial` in a fixed order: lane l adds rows l, l + 64, ... in order, then the butterfly.
__global__ __launch_bounds__(64) void k_expect_final(const double *__restrict__ partial, int rows, int kt, double *__restrict__ out) {
    const int k = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < rows; r += 64) s += partial[(size_t)r * kt + k];
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (threadIdx.x == 0) out[k] = s;
}

template <typename R, bool PAIRED, int KT>
hipError_t launch_kt(hipStream_t stream, const void *a, const void *b, const SweepGeom &g, const ExpectSweep &sw, double *d_partial,
                     double *d_out) {
    TermRec<KT> rec{};
    for (int k = 0; k < sw.count && k < KT; k++) rec.z[k] = sw.z[k];
    rec.im = sw.im_mask;
    constexpr uint64_t per_block = (uint64_t)kTPB * (PAIRED ? 4 : 8);
    // a fixed grid that is resident at once: every workgroup walks the same number of trips, so a second, partly filled round
    // of workgroups would cost a whole round (the 32-slot instantiations hold 3 workgroups per CU, the others 4 and more)
    static const int resident = [] {
        int dev = 0, per_cu = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_expect<R, PAIRED, KT>, kTPB, 0) != hipSuccess || per_cu < 1)
            return kExpectGrid;
        const long r = (long)per_cu * prop.multiProcessorCount;
        return (int)(r < kExpectGrid ? r : kExpectGrid);
    }();
    uint64_t grid = (g.units + per_block - 1) / per_block;
    if (grid > (uint64_t)resident) grid = resident;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL((k_expect<R, PAIRED, KT>), dim3((unsigned)grid), dim3(kTPB), 0, stream, (const R *)a, (const R *)b, g, rec, d_partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_expect_final, dim3(KT), dim3(64), 0, stream, (const double *)d_partial, (int)grid, KT, d_out);
    return hipGetLastError();
}

template <typename R, bool PAIRED>
hipError_t launch_prec(hipStream_t stream, const void *a, const void *b, const SweepGeom &g, const ExpectSweep &sw, double *d_partial, double *d_out) {
    switch (expect_slots(sw.count)) {
    case 1: return launch_kt<R, PAIRED, 1>(stream, a, b, g, sw, d_partial, d_out);
    case 8: return launch_kt<R, PAIRED, 8>(stream, a, b, g, sw, d_partial, d_out);
    case 16: return launch_kt<R, PAIRED, 16>(stream, a, b, g, sw, d_partial, d_out);
    case 32: return launch_kt<R, PAIRED, 32>(stream, a, b, g, sw, d_partial, d_out);
    default: return hipErrorInvalidValue;
    }
}

} // namespace

int expect_slots(int count) { return count <= 1 ? 1 : count <= 8 ? 8 : count <= 16 ? 16 : count <= kMaxTermsPerSweep ? 32 : 0; }

hipError_t launch_expect(const LaunchCfg &cfg, const void *a, const void *b, bool f32, int n, const ExpectSweep &sw, double *d_partial,
                         double *d_out) {
    if (sw.count < 1 || sw.count > kMaxTermsPerSweep || n < 0 || n > 40) return hipErrorInvalidValue;
    const uint64_t N = 1ULL << n;
    if (sw.x >= N) return hipErrorInvalidValue; // the partner index must stay inside the buffer
    const bool paired = sw.x != 0 || sw.full;
    const int as = f32 ? 1 : 0; // log2 amplitudes per unit
    SweepGeom g{};
    g.x = sw.x;
    g.amps = N;
    g.odd_slot = 1;
    g.low = ~0ULL;
    uint64_t amps_visited = N;
    if (sw.x != 0 && !sw.full) { // one member of each pair: the index with the highest bit of x clear
        const int h = 63 - __builtin_clzll(sw.x);
        amps_visited = N >> 1;
        if (h >= as) g.low = (1ULL << (h - as)) - 1ULL; // the zero is inserted at unit bit h - as
        else g.odd_slot = 0;                            // fp32, x == 1: both members share a unit; every unit, even slot only
    }
    g.units = g.odd_slot ? (amps_visited >> as) : N >> as;
    if (g.units == 0) g.units = 1; // one fp32 amplitude
    if (f32) return paired ? launch_prec<float, true>(cfg.stream, a, b, g, sw, d_partial, d_out) : launch_prec<float, false>(cfg.stream, a, b, g, sw, d_partial, d_out);
    return paired ? launch_prec<double, true>(cfg.stream, a, b, g, sw, d_partial, d_out) : launch_prec<double, false>(cfg.stream, a, b, g, sw, d_partial, d_out);
}

} // namespace qsim
