// diagonal.hip — whole-register diagonal operators from a real fp64 table d[0..2^n) on the device (gfx950):
//     k_diag_phase       a_i <- exp(-i gamma d_i) a_i, in place, one sweep: read psi and d, write psi
//     k_diag_expect      sum_i d_i |a_i|^2 and sum_i d_i^2 |a_i|^2, read-only, one sweep
//     k_diag_add_terms   d_i <- d_i + c_0 s_0(i) + c_1 s_1(i) + ..., added in the caller's order, s_k(i) = (-1)^popcount(i & z_k)
//     k_diag_extrema     min, argmin, max, argmax of the table, ties to the lowest index
//     k_diag_adjoint     the backward sweep of an adjoint gradient through exp(-i gamma D): sum_i d_i Im(conj(lam_i) psi_i), and psi
//                        and lambda stepped back, one sweep: read psi, lambda and d, write psi and lambda
//     k_diag_apply       dst_i (= | +=) w d_i src_i, out of place: the diagonal part of lambda = H psi
// Its own object, like combine.hip: nothing here is compiled into kernels.hip.  diagonal.h has the work item and the geometry;
// diagonal.cpp is the host side.
//
// Accesses.  Every global access of the main path is 16 bytes per lane, consecutive lanes on consecutive addresses.  fp32: a state
// unit (two amplitudes) and the table unit of the same two indices belong to one lane.  fp64: a table unit covers two state units, so
// a wave takes a block of 128 amplitudes — lane l loads state units l and 64 + l of the block and table unit l, which holds the
// entries of amplitudes 2l and 2l + 1 — and two 64-bit lane shuffles (table_to_lanes) hand every lane the two entries of its own
// amplitudes.  The shuffles are register moves through the LDS crossbar; no LDS is allocated.  A block needs 64 items, so a register
// of fewer (n <= 6) takes the plain path: one thread per amplitude, 8-byte table loads, one workgroup.  That path also serves the
// registers that have no 16-byte unit: one amplitude is 16 bytes of fp64 state or 8 of fp32, and 8 bytes of table.
//
// The phase factor is formed in fp64 in both precisions — sincospi of (gamma / pi) d_i, whose argument reduction is exact for any
// magnitude — rounded once to the state's precision, and multiplied in that precision with fma (rotate_diag: the x == 0 rule of
// k_pauli_rot with c = cos, sv = -sin).  Every amplitude and every table entry is written by exactly one thread; no atomics.
// The reductions are k_expect's: wave butterfly, waves in order through LDS, one row per workgroup, then a fixed-order final pass.
#include "diagonal.h"

namespace qsim {
namespace {

template <typename R> struct Amp;
template <> struct Amp<double> { using type = double2; };
template <> struct Amp<float> { using type = float2; };

template <typename R>
__device__ __forceinline__ void phase_amp(R &ar, R &ai, double dv, double gamma_over_pi) {
    double sn, cs;
    sincospi(gamma_over_pi * dv, &sn, &cs);
    rotate_diag(ar, ai, (R)cs, (R)-sn);
}

// fp64: lane l of a wave holds table unit l of the wave's block, td = (d[2l], d[2l + 1]); it needs d0 = d[l] and d1 = d[64 + l], the
// entries of its state units.  Lanes below 32 offer (x, y) as (r1, r2), the others (y, x), so that one shuffle of r1 and one of r2
// bring every lane one entry each: an even lane reads r1 of lane l/2 and r2 of lane 32 + l/2, an odd lane the other way round.
// Every lane of the wave must get here.
__device__ __forceinline__ void table_to_lanes(const double2 &td, uint32_t lane, double &d0, double &d1) {
    const bool hi = lane >= 32, odd = lane & 1u;
    const double r1 = hi ? td.y : td.x, r2 = hi ? td.x : td.y;
    const int lo_src = (int)(lane >> 1), hi_src = 32 + (int)(lane >> 1);
    const double s1 = __shfl(r1, odd ? hi_src : lo_src, 64);
    const double s2 = __shfl(r2, odd ? lo_src : hi_src, 64);
    d0 = odd ? s2 : s1;
    d1 = odd ? s1 : s2;
}

// the (even) amplitude a lane's first state unit of item t starts at: fp32 the item's own; fp64 unit `lane` of the wave's block
template <typename R>
__device__ __forceinline__ uint64_t first_amp(uint64_t t, uint32_t lane) {
    if constexpr (sizeof(R) == 4) return 2 * t;
    else return 2 * (t & ~(uint64_t)(kDiagWave - 1)) + lane;
}

template <typename R>
__global__ __launch_bounds__(kTPB) void k_diag_phase(R *a, const double *__restrict__ d, DiagGeom g, double gamma_over_pi) {
    using V = typename Vec16<R>::type;
    using P = typename Amp<R>::type;
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int U = diag_items_per_trip(F32), S = F32 ? 1 : 2; // state units per item
    const uint32_t tid = threadIdx.x, lane = tid & 63u;

    if (g.items < (uint64_t)kDiagWave) { // the plain path: one thread per amplitude
        if (blockIdx.x == 0 && tid < g.amps) {
            P v = *reinterpret_cast<const P *>(a + 2 * tid);
            phase_amp(v.x, v.y, d[tid], gamma_over_pi);
            *reinterpret_cast<P *>(a + 2 * tid) = v;
        }
        return;
    }

    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.items; q0 += (uint64_t)gridDim.x * U) {
        V sv[U][S];
        double2 td[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            td[u] = double2{};
#pragma unroll
            for (int s = 0; s < S; s++) sv[u][s] = V{};
            if (t < g.items) { // uniform over a wave: items is a multiple of 64
                td[u] = *reinterpret_cast<const double2 *>(d + 2 * t);
#pragma unroll
                for (int s = 0; s < S; s++) sv[u][s] = load_unit(const_cast<const R *>(a), first_amp<R>(t, lane) + (uint64_t)kDiagWave * s);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            if constexpr (F32) {
                phase_amp(sv[u][0].x, sv[u][0].y, td[u].x, gamma_over_pi);
                phase_amp(sv[u][0].z, sv[u][0].w, td[u].y, gamma_over_pi);
            } else {
                double d0, d1;
                table_to_lanes(td[u], lane, d0, d1);
                phase_amp(sv[u][0].x, sv[u][0].y, d0, gamma_over_pi);
                phase_amp(sv[u][1].x, sv[u][1].y, d1, gamma_over_pi);
            }
            if (t >= g.items) continue;
#pragma unroll
            for (int s = 0; s < S; s++) *reinterpret_cast<V *>(a + 2 * (first_amp<R>(t, lane) + (uint64_t)kDiagWave * s)) = sv[u][s];
        }
    }
}

// acc0 += dv |a|^2, acc1 += dv^2 |a|^2; the squares of fp32 components are exact in fp64
__device__ __forceinline__ void moments(double &acc0, double &acc1, double re, double im, double dv) {
    const double w = fma(re, re, im * im);
    acc0 = fma(dv, w, acc0);
    acc1 = fma(dv * dv, w, acc1);
}

template <typename R>
__global__ __launch_bounds__(kTPB) void k_diag_expect(const R *__restrict__ a, const double *__restrict__ d, DiagGeom g, double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    using P = typename Amp<R>::type;
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int U = diag_items_per_trip(F32), S = F32 ? 1 : 2;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;

    double acc0 = 0.0, acc1 = 0.0;
    if (g.items < (uint64_t)kDiagWave) { // the plain path: one workgroup, one thread per amplitude
        if (tid < g.amps) {
            const P v = *reinterpret_cast<const P *>(a + 2 * tid);
            moments(acc0, acc1, (double)v.x, (double)v.y, d[tid]);
        }
    } else {
        for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.items; q0 += (uint64_t)gridDim.x * U) {
            V sv[U][S];
            double2 td[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t t = ((q0 + u) << kTidBits) | tid;
                td[u] = double2{};
#pragma unroll
                for (int s = 0; s < S; s++) sv[u][s] = V{};
                if (t < g.items) {
                    td[u] = *reinterpret_cast<const double2 *>(d + 2 * t);
#pragma unroll
                    for (int s = 0; s < S; s++) sv[u][s] = load_unit(a, first_amp<R>(t, lane) + (uint64_t)kDiagWave * s);
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) { // a unit that was not loaded is zeros against table entries of zero: it adds nothing
                if constexpr (F32) {
                    moments(acc0, acc1, (double)sv[u][0].x, (double)sv[u][0].y, td[u].x);
                    moments(acc0, acc1, (double)sv[u][0].z, (double)sv[u][0].w, td[u].y);
                } else {
                    double d0, d1;
                    table_to_lanes(td[u], lane, d0, d1);
                    moments(acc0, acc1, sv[u][0].x, sv[u][0].y, d0);
                    moments(acc0, acc1, sv[u][1].x, sv[u][1].y, d1);
                }
            }
        }
    }

    __shared__ double part[kTPB / 64][2];
    for (int m = 32; m >= 1; m >>= 1) {
        acc0 += __shfl_xor(acc0, m, 64);
        acc1 += __shfl_xor(acc1, m, 64);
    }
    if (lane == 0) part[tid >> 6][0] = acc0, part[tid >> 6][1] = acc1;
    __syncthreads();
    if (tid < 2) {
        double s = 0.0;
        for (int w = 0; w < kTPB / 64; w++) s += part[w][tid];
        partial[(uint64_t)blockIdx.x * 2 + tid] = s;
    }
}

// ---- the backward sweep of an adjoint gradient through exp(-i gamma D) --------------------------------------------------
// acc += dv Im(conj(lam) psi) from the values as they come in, then both amplitudes times ONE factor: phase_amp's, formed once and
// rounded once, so psi is stepped exactly as k_diag_phase would step it.  The components of an fp32 state are widened first: each
// product is then exact and their difference rounds once.
template <typename R>
__device__ __forceinline__ void adjoint_amp(double &acc, R &pr, R &pi, R &lr, R &li, double dv, double gamma_over_pi) {
    acc = fma(dv, fma((double)lr, (double)pi, -((double)li * (double)pr)), acc);
    double sn, cs;
    sincospi(gamma_over_pi * dv, &sn, &cs);
    const R c = (R)cs, sv = (R)-sn;
    rotate_diag(pr, pi, c, sv);
    rotate_diag(lr, li, c, sv);
}

template <typename R>
__global__ __launch_bounds__(kTPB) void k_diag_adjoint(R *psi, R *lam, const double *__restrict__ d, DiagGeom g, double gamma_over_pi,
                                                      double *__restrict__ partial) {
    using V = typename Vec16<R>::type;
    using P = typename Amp<R>::type;
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int U = diag_adjoint_items_per_trip(F32), S = F32 ? 1 : 2;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;

    double acc = 0.0;
    if (g.items < (uint64_t)kDiagWave) { // the plain path: one workgroup, one thread per amplitude
        if (blockIdx.x == 0 && tid < g.amps) {
            P pv = *reinterpret_cast<const P *>(psi + 2 * tid), lv = *reinterpret_cast<const P *>(lam + 2 * tid);
            adjoint_amp(acc, pv.x, pv.y, lv.x, lv.y, d[tid], gamma_over_pi);
            *reinterpret_cast<P *>(psi + 2 * tid) = pv;
            *reinterpret_cast<P *>(lam + 2 * tid) = lv;
        }
    } else {
        for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.items; q0 += (uint64_t)gridDim.x * U) {
            V pv[U][S], lv[U][S];
            double2 td[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t t = ((q0 + u) << kTidBits) | tid;
                td[u] = double2{};
#pragma unroll
                for (int s = 0; s < S; s++) pv[u][s] = V{}, lv[u][s] = V{};
                if (t < g.items) { // uniform over a wave: items is a multiple of 64
                    td[u] = *reinterpret_cast<const double2 *>(d + 2 * t);
#pragma unroll
                    for (int s = 0; s < S; s++) {
                        const uint64_t amp = first_amp<R>(t, lane) + (uint64_t)kDiagWave * s; // psi and lambda at the same index
                        pv[u][s] = load_unit(const_cast<const R *>(psi), amp);
                        lv[u][s] = load_unit(const_cast<const R *>(lam), amp);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) { // a unit that was not loaded is zeros against table entries of zero: it adds nothing
                const uint64_t t = ((q0 + u) << kTidBits) | tid;
                if constexpr (F32) {
                    adjoint_amp(acc, pv[u][0].x, pv[u][0].y, lv[u][0].x, lv[u][0].y, td[u].x, gamma_over_pi);
                    adjoint_amp(acc, pv[u][0].z, pv[u][0].w, lv[u][0].z, lv[u][0].w, td[u].y, gamma_over_pi);
                } else {
                    double d0, d1;
                    table_to_lanes(td[u], lane, d0, d1);
                    adjoint_amp(acc, pv[u][0].x, pv[u][0].y, lv[u][0].x, lv[u][0].y, d0, gamma_over_pi);
                    adjoint_amp(acc, pv[u][1].x, pv[u][1].y, lv[u][1].x, lv[u][1].y, d1, gamma_over_pi);
                }
                if (t >= g.items) continue;
#pragma unroll
                for (int s = 0; s < S; s++) {
                    const uint64_t amp = first_amp<R>(t, lane) + (uint64_t)kDiagWave * s;
                    *reinterpret_cast<V *>(psi + 2 * amp) = pv[u][s];
                    *reinterpret_cast<V *>(lam + 2 * amp) = lv[u][s];
                }
            }
        }
    }

    __shared__ double part[kTPB / 64];
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (lane == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < kTPB / 64; w++) s += part[w];
        partial[blockIdx.x] = s;
    }
}

// ---- dst (= | +=) w D src: the diagonal part of lambda = H psi -------------------------------------------------------------------------
// w dv in fp64, rounded once to the state's precision, times the amplitude (accumulating: one fma per component)
template <typename R, bool ACC>
__device__ __forceinline__ void apply_amp(R &dr, R &di, R sr, R si, double dv, double weight) {
    const R f = (R)(weight * dv);
    if constexpr (ACC) dr = fma(f, sr, dr), di = fma(f, si, di);
    else dr = f * sr, di = f * si;
}

// ACC == false: dst is not loaded.  Items per trip by diagonal.h's rule: the streams of k_diag_phase, or with dst those of k_diag_adjoint.
template <typename R, bool ACC>
__global__ __launch_bounds__(kTPB) void k_diag_apply(const R *__restrict__ src, R *__restrict__ dst, const double *__restrict__ d, DiagGeom g, double weight) {
    using V = typename Vec16<R>::type;
    using P = typename Amp<R>::type;
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int U = ACC ? diag_adjoint_items_per_trip(F32) : diag_items_per_trip(F32), S = F32 ? 1 : 2;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;

    if (g.items < (uint64_t)kDiagWave) { // the plain path: one thread per amplitude
        if (blockIdx.x == 0 && tid < g.amps) {
            const P sv = *reinterpret_cast<const P *>(src + 2 * tid);
            P dv{};
            if constexpr (ACC) dv = *reinterpret_cast<const P *>(dst + 2 * tid);
            apply_amp<R, ACC>(dv.x, dv.y, sv.x, sv.y, d[tid], weight);
            *reinterpret_cast<P *>(dst + 2 * tid) = dv;
        }
        return;
    }

    for (uint64_t q0 = (uint64_t)blockIdx.x * U; (q0 << kTidBits) < g.items; q0 += (uint64_t)gridDim.x * U) {
        V sv[U][S], dv[U][S];
        double2 td[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            td[u] = double2{};
#pragma unroll
            for (int s = 0; s < S; s++) sv[u][s] = V{}, dv[u][s] = V{};
            if (t < g.items) { // uniform over a wave: items is a multiple of 64
                td[u] = *reinterpret_cast<const double2 *>(d + 2 * t);
#pragma unroll
                for (int s = 0; s < S; s++) {
                    const uint64_t amp = first_amp<R>(t, lane) + (uint64_t)kDiagWave * s;
                    sv[u][s] = load_unit(src, amp);
                    if constexpr (ACC) dv[u][s] = load_unit(const_cast<const R *>(dst), amp);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            if constexpr (F32) {
                apply_amp<R, ACC>(dv[u][0].x, dv[u][0].y, sv[u][0].x, sv[u][0].y, td[u].x, weight);
                apply_amp<R, ACC>(dv[u][0].z, dv[u][0].w, sv[u][0].z, sv[u][0].w, td[u].y, weight);
            } else {
                double d0, d1;
                table_to_lanes(td[u], lane, d0, d1);
                apply_amp<R, ACC>(dv[u][0].x, dv[u][0].y, sv[u][0].x, sv[u][0].y, d0, weight);
                apply_amp<R, ACC>(dv[u][1].x, dv[u][1].y, sv[u][1].x, sv[u][1].y, d1, weight);
            }
            if (t >= g.items) continue;
#pragma unroll
            for (int s = 0; s < S; s++) *reinterpret_cast<V *>(dst + 2 * (first_amp<R>(t, lane) + (uint64_t)kDiagWave * s)) = dv[u][s];
        }
    }
}

// Table entries 2t and 2t + 1 of unit t = (q << kTidBits) | tid: popcount(i & z) = popcount((q << 9) & z), uniform over the
// workgroup, + popcount((tid << 1) & z), the thread's own: one bit per term, formed once before the loop, + bit 0 of z for the odd
// entry.  c s is a sign flip of c, exact, and the additions run in the terms' order, so the result is the sequential sum bit for bit.
__global__ __launch_bounds__(kTPB) void k_diag_add_terms(double *d, DiagGeom g, DiagTerms terms) {
    constexpr int E = kDiagAddUnitsPerTrip;
    const uint32_t tid = threadIdx.x;

    if (g.amps < 2) { // a table of one entry is 8 bytes long, no unit; no index bit: s = 1
        if (blockIdx.x == 0 && tid == 0) {
            double v = d[0];
            for (int k = 0; k < terms.count; k++) v += terms.c[k];
            d[0] = v;
        }
        return;
    }

    const uint64_t jl = (uint64_t)tid << 1;
    uint32_t own = 0;
    for (int k = 0; k < terms.count; k++) own |= ((uint32_t)__builtin_popcountll(jl & terms.z[k]) & 1u) << k;

    for (uint64_t q0 = (uint64_t)blockIdx.x * E; (q0 << kTidBits) < g.items; q0 += (uint64_t)gridDim.x * E) {
        double2 v[E];
#pragma unroll
        for (int u = 0; u < E; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            v[u] = double2{};
            if (t < g.items) v[u] = *reinterpret_cast<const double2 *>(d + 2 * t);
        }
        for (int k = 0; k < terms.count; k++) { // uniform: the term's record comes through scalar loads
            const uint64_t z = terms.z[k];
            const double c = terms.c[k];
            const uint32_t mine = ((own >> k) & 1u) << 31;
#pragma unroll
            for (int u = 0; u < E; u++) {
                const uint32_t sg = parity_sign((q0 + u) << (kTidBits + 1), z) ^ mine;
                v[u].x += flip(c, sg);
                v[u].y += flip(c, odd_slot_sign(sg, z));
            }
        }
#pragma unroll
        for (int u = 0; u < E; u++) {
            const uint64_t t = ((q0 + u) << kTidBits) | tid;
            if (t < g.items) *reinterpret_cast<double2 *>(d + 2 * t) = v[u];
        }
    }
}

// ---- extrema: (value, index) pairs, the lower index winning among equal values at every level -------------------------------------
struct Extrema {
    double mn, mx;
    uint64_t imn, imx;
};
__device__ __forceinline__ void take_min(Extrema &e, double v, uint64_t i) {
    if (v < e.mn || (v == e.mn && i < e.imn)) e.mn = v, e.imn = i;
}
__device__ __forceinline__ void take_max(Extrema &e, double v, uint64_t i) {
    if (v > e.mx || (v == e.mx && i < e.imx)) e.mx = v, e.imx = i;
}
__device__ __forceinline__ Extrema no_extrema() { return Extrema{__builtin_inf(), -__builtin_inf(), ~0ULL, ~0ULL}; }
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) { return (uint64_t)__double_as_longlong(__shfl_xor(__longlong_as_double((long long)v), m, 64)); }
__device__ __forceinline__ void wave_extrema(Extrema &e) {
    for (int m = 32; m >= 1; m >>= 1) {
        const double omn = __shfl_xor(e.mn, m, 64), omx = __shfl_xor(e.mx, m, 64);
        const uint64_t oimn = shfl_xor_u64(e.imn, m), oimx = shfl_xor_u64(e.imx, m);
        take_min(e, omn, oimn);
        take_max(e, omx, oimx);
    }
}
// a row of the scratch: min, argmin, max, argmax — the indices as the bits of a double's 8 bytes
__device__ __forceinline__ void store_row(double *row, const Extrema &e) {
    row[0] = e.mn, row[1] = __longlong_as_double((long long)e.imn), row[2] = e.mx, row[3] = __longlong_as_double((long long)e.imx);
}
__device__ __forceinline__ void take_row(Extrema &e, const double *row) {
    take_min(e, row[0], (uint64_t)__double_as_longlong(row[1]));
    take_max(e, row[2], (uint64_t)__double_as_longlong(row[3]));
}

__global__ __launch_bounds__(kTPB) void k_diag_extrema(const double *__restrict__ d, DiagGeom g, double *__restrict__ rows) {
    constexpr int E = kDiagExtremaUnitsPerTrip;
    const uint32_t tid = threadIdx.x;
    Extrema e = no_extrema();
    if (g.amps < 2) { // 8 bytes of table
        if (tid == 0) take_min(e, d[0], 0), take_max(e, d[0], 0);
    } else {
        for (uint64_t q0 = (uint64_t)blockIdx.x * E; (q0 << kTidBits) < g.items; q0 += (uint64_t)gridDim.x * E) {
            double2 v[E];
#pragma unroll
            for (int u = 0; u < E; u++) {
                const uint64_t t = ((q0 + u) << kTidBits) | tid;
                v[u] = double2{};
                if (t < g.items) v[u] = *reinterpret_cast<const double2 *>(d + 2 * t);
            }
#pragma unroll
            for (int u = 0; u < E; u++) {
                const uint64_t t = ((q0 + u) << kTidBits) | tid;
                if (t >= g.items) continue;
                take_min(e, v[u].x, 2 * t), take_max(e, v[u].x, 2 * t);
                take_min(e, v[u].y, 2 * t + 1), take_max(e, v[u].y, 2 * t + 1);
            }
        }
    }
    __shared__ double part[kTPB / 64][kDiagExtremaRowDoubles];
    wave_extrema(e);
    if ((tid & 63u) == 0) store_row(part[tid >> 6], e);
    __syncthreads();
    if (tid == 0) {
        Extrema s = no_extrema();
        for (int w = 0; w < kTPB / 64; w++) take_row(s, part[w]);
        store_row(rows + (uint64_t)blockIdx.x * kDiagExtremaRowDoubles, s);
    }
}

__global__ __launch_bounds__(64) void k_diag_extrema_final(const double *__restrict__ rows, int count, double *__restrict__ out) {
    Extrema e = no_extrema();
    for (int r = threadIdx.x; r < count; r += 64) take_row(e, rows + (size_t)r * kDiagExtremaRowDoubles);
    wave_extrema(e);
    if (threadIdx.x == 0) store_row(out, e);
}

// ---- grids ------------------------------------------------------------------------------------------------------------------------
// A sweep that only writes: QSIM_OPT_GRID_CAP > 0 caps it as it does writing_grid; otherwise what is resident at once, at most `most`.
template <auto Kernel>
unsigned capped_grid(int grid_cap, uint64_t items, uint64_t per_block, int most) {
    const int resident = resident_grid<Kernel>();
    const uint64_t cap = grid_cap > 0 ? (uint64_t)grid_cap : resident > 0 && resident < most ? (uint64_t)resident : (uint64_t)most;
    uint64_t grid = (items + per_block - 1) / per_block;
    if (grid > cap) grid = cap;
    return grid == 0 ? 1u : (unsigned)grid;
}

template <typename R>
hipError_t launch_phase_prec(const LaunchCfg &cfg, void *amps, const DiagGeom &g, const double *table, double gamma_over_pi) {
    const unsigned grid = capped_grid<k_diag_phase<R>>(cfg.grid_cap, g.items, (uint64_t)kTPB * diag_items_per_trip(sizeof(R) == 4), kDiagPhaseGrid);
    hipLaunchKernelGGL((k_diag_phase<R>), dim3(grid), dim3(kTPB), 0, cfg.stream, (R *)amps, table, g, gamma_over_pi);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_expect_prec(hipStream_t stream, const void *amps, const DiagGeom &g, const double *table, double *d_partial, double *d_out) {
    const unsigned grid = reducing_grid<k_diag_expect<R>>(g.items, (uint64_t)kTPB * diag_items_per_trip(sizeof(R) == 4));
    hipLaunchKernelGGL((k_diag_expect<R>), dim3(grid), dim3(kTPB), 0, stream, (const R *)amps, table, g, d_partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_expect_final(stream, d_partial, (int)grid, 2, d_out);
}

// a reducing sweep that also writes: reducing_grid, so cfg.grid_cap does not apply and equal calls return equal bits
template <typename R>
hipError_t launch_adjoint_prec(hipStream_t stream, void *psi, void *lam, const DiagGeom &g, const double *table, double gamma_over_pi, double *d_partial,
                               double *d_out) {
    const unsigned grid = reducing_grid<k_diag_adjoint<R>>(g.items, (uint64_t)kTPB * diag_adjoint_items_per_trip(sizeof(R) == 4));
    hipLaunchKernelGGL((k_diag_adjoint<R>), dim3(grid), dim3(kTPB), 0, stream, (R *)psi, (R *)lam, table, g, gamma_over_pi, d_partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_expect_final(stream, d_partial, (int)grid, 1, d_out);
}

template <typename R, bool ACC>
hipError_t launch_apply_prec(const LaunchCfg &cfg, const void *src, void *dst, const DiagGeom &g, const double *table, double weight) {
    constexpr bool F32 = sizeof(R) == 4;
    constexpr int U = ACC ? diag_adjoint_items_per_trip(F32) : diag_items_per_trip(F32);
    const unsigned grid = capped_grid<k_diag_apply<R, ACC>>(cfg.grid_cap, g.items, (uint64_t)kTPB * U, kDiagPhaseGrid);
    hipLaunchKernelGGL((k_diag_apply<R, ACC>), dim3(grid), dim3(kTPB), 0, cfg.stream, (const R *)src, (R *)dst, table, g, weight);
    return hipGetLastError();
}

} // namespace

hipError_t launch_diag_adjoint(const LaunchCfg &cfg, void *psi, void *lam, bool f32, int n, const double *table, double gamma_over_pi, double *d_partial,
                               double *d_out) {
    if (n < 0 || n > 40 || !psi || !lam || psi == lam || !table || !d_partial || !d_out) return hipErrorInvalidValue;
    const DiagGeom g = diag_geom(n);
    return f32 ? launch_adjoint_prec<float>(cfg.stream, psi, lam, g, table, gamma_over_pi, d_partial, d_out)
               : launch_adjoint_prec<double>(cfg.stream, psi, lam, g, table, gamma_over_pi, d_partial, d_out);
}

hipError_t launch_diag_apply(const LaunchCfg &cfg, const void *src, void *dst, bool f32, int n, const double *table, double weight, bool accumulate) {
    if (n < 0 || n > 40 || !src || !dst || src == dst || !table) return hipErrorInvalidValue;
    const DiagGeom g = diag_geom(n);
    if (f32) return accumulate ? launch_apply_prec<float, true>(cfg, src, dst, g, table, weight) : launch_apply_prec<float, false>(cfg, src, dst, g, table, weight);
    return accumulate ? launch_apply_prec<double, true>(cfg, src, dst, g, table, weight) : launch_apply_prec<double, false>(cfg, src, dst, g, table, weight);
}

hipError_t launch_diag_phase(const LaunchCfg &cfg, void *amps, bool f32, int n, const double *table, double gamma_over_pi) {
    if (n < 0 || n > 40 || !amps || !table) return hipErrorInvalidValue;
    const DiagGeom g = diag_geom(n);
    return f32 ? launch_phase_prec<float>(cfg, amps, g, table, gamma_over_pi) : launch_phase_prec<double>(cfg, amps, g, table, gamma_over_pi);
}

hipError_t launch_diag_expect(const LaunchCfg &cfg, const void *amps, bool f32, int n, const double *table, double *d_partial, double *d_out) {
    if (n < 0 || n > 40 || !amps || !table || !d_partial || !d_out) return hipErrorInvalidValue;
    const DiagGeom g = diag_geom(n);
    return f32 ? launch_expect_prec<float>(cfg.stream, amps, g, table, d_partial, d_out)
               : launch_expect_prec<double>(cfg.stream, amps, g, table, d_partial, d_out);
}

hipError_t launch_diag_add_terms(hipStream_t stream, double *table, int n, const DiagTerms &terms) {
    if (n < 0 || n > 40 || !table || terms.count < 1 || terms.count > kDiagTermsPerRecord) return hipErrorInvalidValue;
    const DiagGeom g = diag_geom(n);
    const unsigned grid = capped_grid<k_diag_add_terms>(0, g.items, (uint64_t)kTPB * kDiagAddUnitsPerTrip, kDiagPhaseGrid);
    hipLaunchKernelGGL(k_diag_add_terms, dim3(grid), dim3(kTPB), 0, stream, table, g, terms);
    return hipGetLastError();
}

hipError_t launch_diag_extrema(hipStream_t stream, const double *table, int n, double *d_scratch) {
    if (n < 0 || n > 40 || !table || !d_scratch) return hipErrorInvalidValue;
    const DiagGeom g = diag_geom(n);
    const unsigned grid = capped_grid<k_diag_extrema>(0, g.items, (uint64_t)kTPB * kDiagExtremaUnitsPerTrip, kDiagExtremaGrid);
    hipLaunchKernelGGL(k_diag_extrema, dim3(grid), dim3(kTPB), 0, stream, table, g, d_scratch);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_diag_extrema_final, dim3(1), dim3(64), 0, stream, (const double *)d_scratch, (int)grid,
                       d_scratch + (size_t)kDiagExtremaGrid * kDiagExtremaRowDoubles);
    return hipGetLastError();
}

} // namespace qsim
