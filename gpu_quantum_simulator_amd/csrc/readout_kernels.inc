// readout_kernels.inc — reductions and gathers that read a state for the host: norm, block probabilities, one masked block.

// k_norm2 has no caller any more: its workgroups' sums meet in one atomicAdd, in whatever order they finish, so equal calls could
// differ in the last bit, and qsim_norm2 (readout.cpp) is now the identity string's expectation sweep, which adds in a fixed order.
// The kernel stays because the code layout of this translation unit is part of what the benchmark measures (DESIGN §3): it leaves
// with the next change that re-measures k_tile.
__global__ __launch_bounds__(TPB) void k_norm2(const amp_t *__restrict__ v, uint64_t N, double *out) {
    double acc = 0.0;
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
        const amp_t a = v[i];
        acc = fma((double)a.x, (double)a.x, fma((double)a.y, (double)a.y, acc));
    }
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    __shared__ double part[TPB / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < TPB / 64; w++) s += part[w];
        atomicAdd(out, s);
    }
}

// Probability mass per block of 2^block_bits amplitudes (measurement post-path).  One workgroup per block; the
// reduction order is fixed (lane-strided partial sums, xor-butterfly inside the wave, waves added in order), so the
// result does not depend on scheduling.
__global__ __launch_bounds__(TPB) void k_block_prob(const amp_t *__restrict__ v, uint64_t N, int block_bits,
                                                    double *__restrict__ out, uint64_t nblocks) {
    __shared__ double part[TPB / 64];
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const uint64_t lo = b << block_bits;
        uint64_t hi = lo + (1ULL << block_bits);
        if (hi > N) hi = N;
        double acc = 0.0;
        for (uint64_t i = lo + threadIdx.x; i < hi; i += TPB) {
            const amp_t a = v[i];
            acc += fma((double)a.x, (double)a.x, (double)a.y * (double)a.y);
        }
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < TPB / 64; w++) t += part[w];
            out[b] = t;
        }
        __syncthreads();
    }
}

// The same sums over blocks that are NOT contiguous: block w holds the amplitudes at deposit(w, hi_mask) | deposit(i,
// lo_mask), i = 0 .. 2^lo_bits - 1 (hi_mask and lo_mask are disjoint sets of index bits).  A sharded state whose qubit
// map was permuted by exchanges keeps a LOGICAL block of the measurement post-path in such a set of local positions, so
// the block sums are formed where the amplitudes are and only the sums travel to the host.  Same fixed reduction order.
__global__ __launch_bounds__(TPB) void k_block_prob_masked(const amp_t *__restrict__ v, uint64_t hi_mask, uint64_t lo_mask, int lo_bits,
                                                           double *__restrict__ out, uint64_t nblocks) {
    __shared__ double part[TPB / 64];
    const uint64_t count = 1ULL << lo_bits;
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const uint64_t base = deposit(b, hi_mask);
        double acc = 0.0;
        for (uint64_t i = threadIdx.x; i < count; i += TPB) {
            const amp_t a = v[base | deposit(i, lo_mask)];
            acc += fma((double)a.x, (double)a.x, (double)a.y * (double)a.y);
        }
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < TPB / 64; w++) t += part[w];
            out[b] = t;
        }
        __syncthreads();
    }
}

// out[i] = v[base | deposit(i, lo_mask)]: one such block, in the order of i, for the host to look inside.
__global__ __launch_bounds__(TPB) void k_gather_masked(const amp_t *__restrict__ v, uint64_t base, uint64_t lo_mask, uint64_t count,
                                                       amp_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < count; i += stride) out[i] = v[base | deposit(i, lo_mask)];
}
