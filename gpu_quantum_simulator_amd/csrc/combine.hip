// combine.hip — linear combinations of whole states with the squared norm of the result from the same sweep (gfx950):
//     dst_i <- d dst_i + a p_i + b q_i,    out[0] = sum_i |dst_i|^2 of the values as STORED
// the one kernel a Lanczos step needs beside lambda = H psi (adjoint.hip) and Re <lambda|psi> (expect.hip), and what qsim_combine
// offers on its own (state_algebra.cpp, lanczos.cpp).  Its own object, like the Pauli sweeps: nothing here is compiled
// into kernels.hip.  pauli_sweep.h says how a sweep walks a state; this one is the plainest of them — x == 0, every 16-byte unit,
// no partner, no parity — so of the shared pieces it uses the geometry, the unit loads and the reducing grid.
//
// Shapes.  A stream that is not used is not loaded: q absent (HAS_Q = false) and d == 0 (LOAD_DST = false: dst may hold anything,
// NaN included — a pure write) are template parameters, four instantiations per precision.  Units per thread and trip follow the
// rule of the other sweeps, 8 independent 16-byte loads in flight: 8 units for one stream (dst <- a p), 4 for two, 3 for three (9
// loads: 2 would leave a quarter of the queue empty).
//
// Arithmetic.  The coefficients are rounded once by the host to the state's precision and the multiply-adds run in that precision,
// as in k_pauli_sum.  The norm is accumulated in fp64 from the rounded values that are stored (a product of two floats is exact in
// fp64), so it is what a norm sweep over dst would give afterwards up to the order of summation.  Reduction: k_expect's — wave
// butterfly, waves added in order through LDS, one row per workgroup, launch_expect_final; no atomics, equal calls give equal bits.
#include "pauli_sweep.h"

namespace qsim {
namespace {

template <typename R>
struct CombineCoef { R dr, di, ar, ai, br, bi; }; // by value: scalar loads

constexpr int combine_units_per_trip(int streams) { return streams == 1 ? 8 : streams == 2 ? 4 : 3; }

// (xr, xi) += (cr + i ci) (vr, vi)
template <typename R>
__device__ __forceinline__ void cmad(R &xr, R &xi, R cr, R ci, R vr, R vi) {
    xr = fma(-ci, vi, fma(cr, vr, xr));
    xi = fma(ci, vr, fma(cr, vi, xi));
}

template <typename R, bool LOAD_DST, bool HAS_Q>
__global__ __launch_bounds__(kTPB) void k_combine(R *dst, const R *__restrict__ p, const R *__restrict__ q, SweepGeom g, CombineCoef<R> c,
                                                  double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    constexpr int A = sizeof(R) == 8 ? 1 : 2; // amplitudes per unit
    constexpr int U = combine_units_per_trip(1 + (LOAD_DST ? 1 : 0) + (HAS_Q ? 1 : 0));
    const uint32_t tid = threadIdx.x;
    const bool tiny = A == 2 && g.amps < 2; // a register of one fp32 amplitude is 8 bytes long

    double acc = 0.0;
    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.units; q0 += (uint64_t)gridDim.x * U) {
        V vd[U], vp[U], vq[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            vd[u] = V{};
            vp[u] = V{};
            vq[u] = V{};
            if (t < g.units) {
                const uint64_t i = expand<R>(g, t);
                vp[u] = load_unit_or_one(g, p, i);
                if (HAS_Q) vq[u] = load_unit_or_one(g, q, i);
                if (LOAD_DST) vd[u] = load_unit_or_one(g, const_cast<const R *>(dst), i);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            if (t >= g.units) continue;
            const uint64_t i = expand<R>(g, t);
            R xr[A], xi[A];
            const R *d = reinterpret_cast<const R *>(&vd[u]), *a = reinterpret_cast<const R *>(&vp[u]), *b = reinterpret_cast<const R *>(&vq[u]);
#pragma unroll
            for (int s = 0; s < A; s++) {
                xr[s] = xi[s] = (R)0;
                if (LOAD_DST) cmad(xr[s], xi[s], c.dr, c.di, d[2 * s], d[2 * s + 1]);
                cmad(xr[s], xi[s], c.ar, c.ai, a[2 * s], a[2 * s + 1]);
                if (HAS_Q) cmad(xr[s], xi[s], c.br, c.bi, b[2 * s], b[2 * s + 1]);
            }
            if constexpr (A == 1) {
                *reinterpret_cast<V *>(dst + 2 * i) = V{xr[0], xi[0]};
                acc += fma(xr[0], xr[0], xi[0] * xi[0]);
            } else {
                if (tiny) *reinterpret_cast<float2 *>(dst) = float2{xr[0], xi[0]};
                else *reinterpret_cast<V *>(dst + 2 * i) = V{xr[0], xi[0], xr[1], xi[1]};
                const double r0 = xr[0], i0 = xi[0], r1 = tiny ? 0.0 : (double)xr[1], i1 = tiny ? 0.0 : (double)xi[1];
                acc += fma(r0, r0, i0 * i0) + fma(r1, r1, i1 * i1);
            }
        }
    }

    __shared__ double part[kTPB / 64];
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < kTPB / 64; w++) s += part[w];
        partial[blockIdx.x] = s;
    }
}

template <typename R, bool LOAD_DST, bool HAS_Q>
hipError_t launch_shape(hipStream_t stream, void *dst, const void *p, const void *q, const SweepGeom &g, const double *d, const double *a,
                        const double *b, double *d_partial, double *d_out) {
    CombineCoef<R> c{};
    if (LOAD_DST) c.dr = (R)d[0], c.di = (R)d[1];
    c.ar = (R)a[0], c.ai = (R)a[1];
    if (HAS_Q) c.br = (R)b[0], c.bi = (R)b[1];
    constexpr int U = combine_units_per_trip(1 + (LOAD_DST ? 1 : 0) + (HAS_Q ? 1 : 0));
    const unsigned grid = reducing_grid<k_combine<R, LOAD_DST, HAS_Q>>(g.units, (uint64_t)kTPB * U);
    hipLaunchKernelGGL((k_combine<R, LOAD_DST, HAS_Q>), dim3(grid), dim3(kTPB), 0, stream, (R *)dst, (const R *)p, (const R *)q, g, c, d_partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_expect_final(stream, d_partial, (int)grid, 1, d_out);
}

template <typename R>
hipError_t launch_prec(hipStream_t stream, void *dst, bool load_dst, const void *p, const void *q, const SweepGeom &g, const double *d, const double *a,
                       const double *b, double *d_partial, double *d_out) {
    if (load_dst) return q ? launch_shape<R, true, true>(stream, dst, p, q, g, d, a, b, d_partial, d_out)
                           : launch_shape<R, true, false>(stream, dst, p, q, g, d, a, b, d_partial, d_out);
    return q ? launch_shape<R, false, true>(stream, dst, p, q, g, d, a, b, d_partial, d_out)
             : launch_shape<R, false, false>(stream, dst, p, q, g, d, a, b, d_partial, d_out);
}

} // namespace

hipError_t launch_combine(const LaunchCfg &cfg, void *dst, const double *d, const void *p, const double *a, const void *q, const double *b, bool f32,
                          int n, double *d_partial, double *d_out) {
    if (n < 0 || n > 40 || !dst || !p || !a || p == dst || q == dst || (q && !b) || !d_partial || !d_out) return hipErrorInvalidValue;
    const bool load_dst = d && (d[0] != 0.0 || d[1] != 0.0);
    const SweepGeom g = sweep_geom(0, false, f32, n); // every unit, nothing inserted
    return f32 ? launch_prec<float>(cfg.stream, dst, load_dst, p, q, g, d, a, b, d_partial, d_out)
               : launch_prec<double>(cfg.stream, dst, load_dst, p, q, g, d, a, b, d_partial, d_out);
}

} // namespace qsim
