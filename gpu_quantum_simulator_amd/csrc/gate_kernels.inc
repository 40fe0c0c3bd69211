// gate_kernels.inc — the streaming kernels: one sweep over the state per launch (initialisation, one gate each).

// |0...0>
__global__ __launch_bounds__(TPB) void k_init(amp_t *__restrict__ v, uint64_t N, double amp0) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride)
        v[i] = amp_t{(real_t)(i == 0 ? amp0 : 0.0), (real_t)0};
}

// Zeroes every amplitude whose index has a bit of zero_mask set: materialises a state that the tile passes have only
// written inside its support so far (qsim_state::support).  Write-only.
__global__ __launch_bounds__(TPB) void k_zero_outside(amp_t *__restrict__ v, uint64_t N, uint64_t zero_mask) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride)
        if (i & zero_mask) v[i] = amp_t{(real_t)0, (real_t)0};
}

// Dense 2x2, target bit q >= 6.  Work item = amplitude pair (i0, i0 | 2^q); consecutive lanes take
// consecutive i0, so each wave-instruction reads/writes one contiguous KiB from each of two streams
// 2^q amplitudes apart.  IPT pairs per thread -> 2*IPT independent 16-B loads in flight per lane.
template <int IPT, bool GUARD>
__global__ __launch_bounds__(TPB) void k_gate1_hi(amp_t *__restrict__ v, uint64_t npairs, int q, M2 U,
                                                  uint64_t ntiles) {
    const uint64_t bit = 1ULL << q;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)(TPB * IPT) + threadIdx.x;
        uint64_t i0[IPT];
        amp_t a0[IPT], a1[IPT];
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t t = t0 + (uint64_t)k * TPB;
            i0[k] = insert_zero(t, q);
            if (!GUARD || t < npairs) {
                a0[k] = v[i0[k]];
                a1[k] = v[i0[k] | bit];
            }
        }
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t t = t0 + (uint64_t)k * TPB;
            if (!GUARD || t < npairs) {
                v[i0[k]] = cfma(a1[k], U.re[1], U.im[1], cmul(a0[k], U.re[0], U.im[0]));
                v[i0[k] | bit] = cfma(a1[k], U.re[3], U.im[3], cmul(a0[k], U.re[2], U.im[2]));
            }
        }
    }
}

// Dense 2x2, target bit q < 6: both amplitudes of a pair sit in the same wave's contiguous KiB.  Each
// lane loads its own amplitude (perfectly coalesced), fetches the partner's with a wave shuffle
// (lane ^ 2^q — the butterfly), and computes its own output row.  Same flops per amplitude as the pair
// form, no second pass, no LDS allocation.
template <int IPT, bool GUARD>
__global__ __launch_bounds__(TPB) void k_gate1_lo(amp_t *__restrict__ v, uint64_t N, int q, M2 U, uint64_t ntiles) {
    const bool up = (threadIdx.x >> q) & 1; // bit q of the amplitude index == bit q of the lane id
    const real_t own_r = up ? U.re[3] : U.re[0], own_i = up ? U.im[3] : U.im[0];
    const real_t par_r = up ? U.re[2] : U.re[1], par_i = up ? U.im[2] : U.im[1];
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * (uint64_t)(TPB * IPT) + threadIdx.x;
        amp_t a[IPT];
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t i = i0 + (uint64_t)k * TPB;
            a[k] = (!GUARD || i < N) ? v[i] : amp_t{(real_t)0, (real_t)0};
        }
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t i = i0 + (uint64_t)k * TPB;
            const amp_t p = shfl_xor2(a[k], 1 << q);
            const amp_t r = cfma(p, par_r, par_i, cmul(a[k], own_r, own_i));
            if (!GUARD || i < N) v[i] = r;
        }
    }
}

// diag(1, lambda): only the bit=1 half is read and written (16*N bytes instead of 32*N).
template <int IPT, bool GUARD>
__global__ __launch_bounds__(TPB) void k_phase(amp_t *__restrict__ v, uint64_t nitems, int q, double lr, double li,
                                               uint64_t ntiles) {
    const uint64_t bit = 1ULL << q;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)(TPB * IPT) + threadIdx.x;
        uint64_t idx[IPT];
        amp_t a[IPT];
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t t = t0 + (uint64_t)k * TPB;
            idx[k] = insert_zero(t, q) | bit;
            if (!GUARD || t < nitems) a[k] = v[idx[k]];
        }
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t t = t0 + (uint64_t)k * TPB;
            if (!GUARD || t < nitems) v[idx[k]] = cmul(a[k], lr, li);
        }
    }
}

// diag(d0, d1) over every amplitude (used when d0 != 1, or when q < 2 makes the half form touch every
// 64-B sector anyway).
template <int IPT, bool GUARD>
__global__ __launch_bounds__(TPB) void k_diag1_full(amp_t *__restrict__ v, uint64_t N, int q, double d0r, double d0i,
                                                    double d1r, double d1i, uint64_t ntiles) {
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * (uint64_t)(TPB * IPT) + threadIdx.x;
        amp_t a[IPT];
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t i = i0 + (uint64_t)k * TPB;
            if (!GUARD || i < N) a[k] = v[i];
        }
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t i = i0 + (uint64_t)k * TPB;
            const bool up = (i >> q) & 1;
            if (!GUARD || i < N) v[i] = cmul(a[k], up ? d1r : d0r, up ? d1i : d0i);
        }
    }
}

// CX: swap v[i | c] <-> v[i | c | t] over the N/4 indices i with both bits clear.
template <int IPT, bool GUARD>
__global__ __launch_bounds__(TPB) void k_cx(amp_t *__restrict__ v, uint64_t nitems, int lo, int hi, uint64_t cbit,
                                            uint64_t tbit, uint64_t ntiles) {
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)(TPB * IPT) + threadIdx.x;
        uint64_t ia[IPT];
        amp_t a[IPT], b[IPT];
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t t = t0 + (uint64_t)k * TPB;
            ia[k] = insert_zero(insert_zero(t, lo), hi) | cbit;
            if (!GUARD || t < nitems) {
                a[k] = v[ia[k]];
                b[k] = v[ia[k] | tbit];
            }
        }
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t t = t0 + (uint64_t)k * TPB;
            if (!GUARD || t < nitems) {
                v[ia[k]] = b[k];
                v[ia[k] | tbit] = a[k];
            }
        }
    }
}

// Dense 4x4 with both target bits >= 6: four coalesced streams, all arithmetic in registers, matrix in
// kernel arguments (scalar registers).  Row/column index = (bit hi, bit lo), row-major
// (quantum_simulator_4x4.cu:119-134).
template <int IPT, bool GUARD>
__global__ __launch_bounds__(TPB) void k_gate2_hh(amp_t *__restrict__ v, uint64_t nitems, int lo, int hi, M4 U,
                                                  uint64_t ntiles) {
    const uint64_t blo = 1ULL << lo, bhi = 1ULL << hi;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = tile * (uint64_t)(TPB * IPT) + threadIdx.x;
        uint64_t i00[IPT];
        amp_t x[IPT][4];
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t t = t0 + (uint64_t)k * TPB;
            i00[k] = insert_zero(insert_zero(t, lo), hi);
            if (!GUARD || t < nitems) {
                x[k][0] = v[i00[k]];
                x[k][1] = v[i00[k] | blo];
                x[k][2] = v[i00[k] | bhi];
                x[k][3] = v[i00[k] | bhi | blo];
            }
        }
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t t = t0 + (uint64_t)k * TPB;
            if (!GUARD || t < nitems) {
                amp_t y[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    amp_t acc = cmul(x[k][0], U.re[4 * r], U.im[4 * r]);
#pragma unroll
                    for (int c = 1; c < 4; c++) acc = cfma(x[k][c], U.re[4 * r + c], U.im[4 * r + c], acc);
                    y[r] = acc;
                }
                v[i00[k]] = y[0];
                v[i00[k] | blo] = y[1];
                v[i00[k] | bhi] = y[2];
                v[i00[k] | bhi | blo] = y[3];
            }
        }
    }
}
