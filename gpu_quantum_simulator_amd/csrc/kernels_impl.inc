// kernels_impl.inc — the kernels and their launchers, generic in the amplitude precision.  Included twice by kernels.hip
// (namespace f64: QSIM_REAL = double, 16-byte amplitudes; namespace f32: QSIM_REAL = float, 8-byte amplitudes — the
// precision of the reference's CUDA variants, quantum_simulator_naive.cu:145-149).  No include guards on purpose.


// Amplitudes travel as clang's native 2 x real vector (fp64: one global_load_dwordx4 / ds_read_b128 each; fp32: dwordx2 /
// b64) and, unlike the HIP_vector_type wrapper, a first-class value (arrays of it stay in registers).
typedef QSIM_REAL real_t;
typedef real_t amp_t __attribute__((ext_vector_type(2)));
constexpr int kAmpShift = QSIM_AMP_SHIFT; // log2(sizeof(amp_t))
static_assert(sizeof(amp_t) == (1u << kAmpShift), "QSIM_AMP_SHIFT must match the amplitude size");

// r = a*u (complex), then r += b*w — written as explicit FMAs so hipcc keeps one v_fma_f64 each.
__device__ __forceinline__ amp_t cmul(amp_t a, real_t ur, real_t ui) {
    amp_t r;
    r.x = fma(a.x, ur, -(a.y * ui));
    r.y = fma(a.x, ui, a.y * ur);
    return r;
}
__device__ __forceinline__ amp_t cfma(amp_t a, real_t ur, real_t ui, amp_t acc) {
    amp_t r;
    r.x = fma(a.x, ur, fma(-a.y, ui, acc.x));
    r.y = fma(a.x, ui, fma(a.y, ur, acc.y));
    return r;
}
__device__ __forceinline__ amp_t shfl_xor2(amp_t a, int mask) {
    amp_t r;
    r.x = __shfl_xor(a.x, mask, 64);
    r.y = __shfl_xor(a.y, mask, 64);
    return r;
}

// ---------------------------------------------------------------------------------------------------
// |0...0>
__global__ __launch_bounds__(TPB) void k_init(amp_t *__restrict__ v, uint64_t N, double amp0) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride)
        v[i] = amp_t{(real_t)(i == 0 ? amp0 : 0.0), (real_t)0};
}

// ---------------------------------------------------------------------------------------------------
// Dense 2x2, target bit q >= 6.  Work item = amplitude pair (i0, i0 | 2^q); consecutive lanes take
// consecutive i0, so each wave-instruction reads/writes one contiguous KiB from each of two streams
// 2^q amplitudes apart.  IPT pairs per thread -> 2*IPT independent 16-B loads in flight per lane.
// Zeroes every amplitude whose index has a bit of zero_mask set: materialises a state that the tile passes have only
// written inside its support so far (qsim_state::support).  Write-only.
__global__ __launch_bounds__(TPB) void k_zero_outside(amp_t *__restrict__ v, uint64_t N, uint64_t zero_mask) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride)
        if (i & zero_mask) v[i] = amp_t{(real_t)0, (real_t)0};
}

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

// ---------------------------------------------------------------------------------------------------
// Cache-blocked pass.  A tile is the 2^B amplitudes that agree on every index bit outside the tile set
// T = {0..L-1} U {high[0..H-1]}; it is 2^H contiguous runs of 2^L amplitudes (16*2^L bytes each), so
// global traffic stays in whole-KiB pieces whatever the high qubits are.  One workgroup stages a tile
// in LDS, applies the whole op list to it (every op's qubits lie in T), and writes it back: one read
// and one write of the state for n_ops fused blocks.  Op matrices are read with wave-uniform
// addresses from a const __restrict__ buffer (scalar loads through the constant cache).
//
// Inside the tile an op on local bit b pairs LDS slots (i, i | 2^b); each pair/quad is owned by one
// thread, so only a workgroup barrier between ops is needed.
// Geometry as the kernel sees it: the high tile bits as a mask (no runtime-indexed arrays in device code).
struct TileDev {
    int32_t tile_bits, low_bits, n_high, n;
    int32_t from_zero_ket; // 1: the state is a basis state that has not been written yet: generate it, do not load it
    double amp0;                // its amplitude at index 0 (1 for |0...0>, 0 for a shard that does not hold index 0)
    uint64_t high_mask; // global bit positions of tile-local bits L..B-1 (as a set)
    uint64_t zero_mask; // index bits the state is known to be |0> in (qsim_state::support): amplitudes with such a bit set are
                        // zero BY DEFINITION — their memory has never been written — so tiles with one in their base index are
                        // not visited at all and, inside the visited tiles, such slots are staged in as zero WITHOUT being loaded
    int32_t live_regs;  // k_tile<SPARSE>: registers 0 .. live_regs-1 of a lane hold slots inside the support; the others sit on tile bits
                        // in zero_mask that the engine placed in the topmost register role (place_new_bits) and are never loaded
    int8_t high[16];    // ... and in order: tile-local bit L+j is global bit high[j].  ANY order: which tile bits the lanes of a
                        // wave, the waves of a workgroup and the registers of a lane walk is the engine's choice
};

// software PDEP: spreads the low bits of x over the set bits of mask, lowest first
__device__ __forceinline__ uint64_t deposit(uint64_t x, uint64_t mask) {
    uint64_t out = 0;
    while (mask) {
        const uint64_t low = mask & (0 - mask);
        if (x & 1ULL) out |= low;
        x >>= 1;
        mask &= mask - 1;
    }
    return out;
}

// Op data is read through the CONSTANT address space with wave-uniform addresses, so hipcc emits scalar
// loads (s_load_dwordx*): the matrix lives in SGPRs / the scalar cache, not in vector registers.
typedef const TileOp __attribute__((address_space(4))) *ConstOps;

// LDS layout swizzle of a tile slot index (qsim_internal.h lds_sw_fold: one definition for the kernels and the encoder)
constexpr int kSwLow = kLdsSwLow<kAmpShift>; // slot bits below this are the unit inside a bank row
__device__ __forceinline__ uint32_t sw_slot(uint32_t slot) { return slot ^ lds_sw_fold<kAmpShift>(slot >> kSwLow); }
__device__ __forceinline__ uint32_t sw_byte(uint32_t byte) { return byte ^ (lds_sw_fold<kAmpShift>(byte >> (kSwLow + kAmpShift)) << kAmpShift); }

// LDS access by raw byte address.  k_tile has no static __shared__, so its dynamic LDS region starts at address 0
// (AMDGPU ABI: dynamic LDS follows the static part) and a tile byte offset IS the LDS address; going through the
// `extern __shared__` symbol instead costs one v_add_u32 (of a link-time zero) per access.
typedef __attribute__((address_space(3))) amp_t lds_amp_t;
__device__ __forceinline__ amp_t lds_load(uint32_t byte) { return *(lds_amp_t *)(uintptr_t)byte; }
__device__ __forceinline__ void lds_put(uint32_t byte, amp_t v) { *(lds_amp_t *)(uintptr_t)byte = v; }

// Index of the k-th work item with a zero inserted at bit b (b wave-uniform): x + (x & ~((1<<b)-1)).
// Op coefficients are stored in the state's precision (the engine rounds once and packs them the way the kernels read them,
// tile_op.cpp), and they arrive through scalar loads either way.
typedef const __attribute__((address_space(4))) real_t *ConstCoef;
typedef const PartRec __attribute__((address_space(4))) *ConstRec;

// A block coefficient u = ur + i*ui as the tile ops consume it.  fp64: the two scalars (re, im), 16 bytes per entry.  fp32
// (QSIM_COEF_PAIRS): the engine stores every coefficient as the two pairs (ur, ui) and (-ui, ur) — again 16 bytes — so a
// scalar load brings them in as ready-made SGPR pairs and a complex multiply-add is two v_pk_fma_f32
// (a.x * (ur, ui) + a.y * (-ui, ur) + acc) instead of four v_fma_f32: the block phase of an fp32 pass costs as many VALU
// instructions per amplitude as an fp64 one otherwise, and an fp32 pass has half the bytes to hide them behind.
#if QSIM_COEF_PAIRS
struct coef_t { amp_t u1, u2; };
typedef const __attribute__((address_space(4))) amp_t *ConstPair;
__device__ __forceinline__ coef_t rec_coef(ConstRec rec, int e) { return coef_t{((ConstPair)rec->coef)[2 * e], ((ConstPair)rec->coef)[2 * e + 1]}; }
__device__ __forceinline__ coef_t make_coef(real_t r, real_t i) { return coef_t{amp_t{r, i}, amp_t{-i, r}}; }
__device__ __forceinline__ amp_t cmul(amp_t a, coef_t c) {
    return __builtin_elementwise_fma(amp_t{a.x, a.x}, c.u1, amp_t{a.y, a.y} * c.u2);
}
__device__ __forceinline__ amp_t cfma(amp_t a, coef_t c, amp_t acc) {
    return __builtin_elementwise_fma(amp_t{a.x, a.x}, c.u1, __builtin_elementwise_fma(amp_t{a.y, a.y}, c.u2, acc));
}
#else
struct coef_t { real_t r, i; };
__device__ __forceinline__ coef_t rec_coef(ConstRec rec, int e) { return coef_t{((ConstCoef)rec->coef)[2 * e], ((ConstCoef)rec->coef)[2 * e + 1]}; }
__device__ __forceinline__ coef_t make_coef(real_t r, real_t i) { return coef_t{r, i}; }
__device__ __forceinline__ amp_t cmul(amp_t a, coef_t c) { return cmul(a, c.r, c.i); }
__device__ __forceinline__ amp_t cfma(amp_t a, coef_t c, amp_t acc) { return cfma(a, c.r, c.i, acc); }
#endif

__device__ __forceinline__ uint32_t ins0(uint32_t x, uint32_t himask) { return x + (x & himask); }

// First 16 bytes of a TileOp as four dwords through one scalar load (layout: qsim_internal.h).
typedef uint32_t OpHeader __attribute__((ext_vector_type(4)));
__device__ __forceinline__ OpHeader op_header(ConstOps ops, int oi) {
    return *(const __attribute__((address_space(4))) OpHeader *)(ops + oi);
}
// the bank a tile gets from the block's qubits outside the tile (wave-uniform: a workgroup is on one tile)
__device__ __forceinline__ int op_bank(const OpHeader h, uint64_t tile_base) {
    const uint32_t nsel = h[0] >> 24;
    if (nsel == 0) return 0;
    int bank = (int)((tile_base >> (h[1] & 255u)) & 1ULL);
    if (nsel > 1) bank = 2 * bank + (int)((tile_base >> ((h[1] >> 8) & 255u)) & 1ULL);
    return bank;
}

// Scalar loads of a part record, placed by hand.  Left to the compiler, every scalar load of a part floats to the top of the
// block (they are invariant loads: nothing orders them) — 128 coefficient SGPRs at T = 4, more than a wave has — and what does
// not fit is spilled to VGPR lanes and read back (v_writelane / v_readlane on the vector pipe: 186 spilled SGPRs, 32 + 40 such
// instructions per block, measured in the ISA), and scheduling fences do not hold them (they are placed before the scheduler
// runs).  As volatile asm statements they stay where they are written, in batches that fit the scalar file; the wait that
// follows a batch names the loaded registers as in/out operands, so nothing that uses them can move in front of it.  The
// compiler's own s_waitcnt bookkeeping does not see these loads; that only makes its LDS waits conservative (LDS reads return in
// order, and an outstanding scalar load can only keep the counter higher), and every batch is drained with lgkmcnt(0) here.
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
template <int BYTE>
__device__ __forceinline__ u32x16 sload16(ConstRec rec) {
    u32x16 v;
    asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(v) : "s"(rec), "n"(BYTE));
    return v;
}
template <int BYTE>
__device__ __forceinline__ u32x8 sload8(ConstRec rec) {
    u32x8 v;
    asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(v) : "s"(rec), "n"(BYTE));
    return v;
}
// entry j of a coefficient row held in SGPRs: dwords 4j .. 4j+3 (fp64: re, im; fp32: the pairs (ur, ui), (-ui, ur))
template <typename V>
__device__ __forceinline__ coef_t sgpr_coef(const V &v, int j) {
#if QSIM_COEF_PAIRS
    // (the dwords are copied to scalars first: __builtin_bit_cast applied to a vector ELEMENT expression reads element 0 for
    // every index with this compiler — found by the fp32 parity tests, reproduced in isolation)
    const uint32_t w0 = v[4 * j], w1 = v[4 * j + 1], w2 = v[4 * j + 2], w3 = v[4 * j + 3];
    return coef_t{amp_t{__uint_as_float(w0), __uint_as_float(w1)}, amp_t{__uint_as_float(w2), __uint_as_float(w3)}};
#else
    return coef_t{__builtin_bit_cast(double, (uint64_t)v[4 * j] | ((uint64_t)v[4 * j + 1] << 32)),
                  __builtin_bit_cast(double, (uint64_t)v[4 * j + 2] | ((uint64_t)v[4 * j + 3] << 32))};
#endif
}
constexpr int kRecCoefByte = 2 * kPartRows * 4; // offsetof(PartRec, coef)

// One TOP_PART block (qsim_internal.h): every lane owns one (group, part) = 8 positions of the block, i.e. 8 / T whole classes;
// the parts of a group are dealt part-major, so a wave works on ONE part and everything it needs of the block is the one
// wave-uniform record `rec`: all scalar loads are at immediate offsets from that pointer.  All loop bounds static.
// Order of work per item:
//   T = 1, 2:  [offsets, row offsets, ALL coefficients of the part: 48 / 80 SGPRs] wait  [the 8 LDS reads]  multiply-adds
//   T = 4:     [offsets, class 0's coefficients: 72 SGPRs] wait  [the 8 LDS reads]  multiply-adds of class 0
//              [row offsets, class 1's coefficients into the same registers] wait  multiply-adds of class 1
//   then a barrier if other waves read what this one writes, and the 8 LDS writes.
// What a block needs before its first load: the part record of each of the lane's items and the LDS byte address of the item's group.
template <int B, int THREADS>
struct PartPlan {
    static constexpr uint32_t ITEMS = (1u << B) / kPartRows;
    static constexpr int IPT = ITEMS >= (uint32_t)THREADS ? ITEMS / THREADS : 1;
    ConstRec rec[IPT];
    uint32_t base[IPT];
    uint32_t info; // bit 0: run (the tile's bank is not the identity), bits 1-2: log2 T, bit 3: skips, bit 4: barrier between reads and writes
};
// The tile-independent half: which part each of the lane's items belongs to and where its group starts in LDS.
template <int B, int THREADS>
__device__ __forceinline__ void part_geometry(uint32_t lds_base, const OpHeader h, uint32_t tid, int *part, uint32_t *base) {
    const int K = (int)((h[0] >> 8) & 255u);
    const uint32_t gbits = (uint32_t)(B - K);  // K > 3 only where B - K >= 6: a part is at least one wave (Scheduler::merge_blocks)
    const int nparts = 1 << (K - 3);
#pragma unroll
    for (int i = 0; i < PartPlan<B, THREADS>::IPT; i++) {
        const uint32_t item = tid + i * THREADS;
        const int p = __builtin_amdgcn_readfirstlane((int)(item >> gbits));
        part[i] = p < nparts ? p : 0; // waves beyond the last item (tiles smaller than 8 * THREADS) stay in bounds
        // Which tile-local bit each bit of the group index lands on is the engine's choice (nibble a of dwords 2-3 of the header, 15
        // for the item bits that select the part): ANY assignment of the block's free bits to the lanes enumerates the groups, and
        // the engine picks one under which the lanes of a ds_read_b128 / ds_write_b128 group fall on different banks (tile_op.cpp).
        uint32_t x = 0;
#pragma unroll
        for (int a = 0; a < (B > 3 ? B - 3 : 0); a++) {
            const uint32_t pos = ((a < 8 ? h[2] >> (4 * a) : h[3] >> (4 * (a - 8))) & 15u); // wave-uniform
            x |= ((item >> a) & 1u) << pos;
        }
        x &= (1u << B) - 1u; // (position 15: the part bits fall off)
        base[i] = lds_base | sw_byte(x << kAmpShift); // buffers are aligned to their size: OR, and the XORed offsets stay inside
    }
}
template <int B, int THREADS>
__device__ __forceinline__ PartPlan<B, THREADS> part_prepare(uint32_t lds_base, ConstOps ops, int oi, const OpHeader h, uint64_t tile_base, uint32_t tid) {
    PartPlan<B, THREADS> pl;
    const int bank = op_bank(h, tile_base);
    pl.info = (((h[1] >> (16 + bank)) & 1u) ^ 1u) | (h[3] >> 24); // the engine packs log2 T, skips and the barrier bit into b[7] in info's positions
    int part[PartPlan<B, THREADS>::IPT];
    part_geometry<B, THREADS>(lds_base, h, tid, part, pl.base);
#pragma unroll
    for (int i = 0; i < PartPlan<B, THREADS>::IPT; i++) pl.rec[i] = &ops[oi].rec[bank][part[i]];
    return pl;
}

template <int B, int THREADS, int T, bool SKIPS>
__device__ __forceinline__ void tile_op_part(const PartPlan<B, THREADS> &pl, uint32_t tid, bool mid_barrier) {
    constexpr uint32_t E = 1u << B;
    constexpr uint32_t ITEMS = E / kPartRows;
    constexpr int IPT = ITEMS >= (uint32_t)THREADS ? ITEMS / THREADS : 1;
    constexpr bool FULL = ITEMS >= (uint32_t)THREADS && ITEMS % THREADS == 0;
    constexpr int NC = kPartRows / T; // classes per part
    static_assert(kRecCoefByte == 64 && sizeof(PartRec) == 64 + 512, "record layout");
    const ConstRec *rec = pl.rec;
    const uint32_t *base = pl.base;
    // Phase 1: every operand of every item of the lane is read.  The barrier that protects them from other waves' writes sits
    // HERE, behind the reads, not behind the arithmetic: the waves arrive together (they left the previous block's barrier
    // together) and wait for a few hundred cycles of LDS latency instead of for the slowest wave's multiply-adds (measured with
    // in-kernel stamps: 760-820 cycles of a 4600-cycle block behind the arithmetic), and the writes of phase 2 then leave
    // the waves one by one instead of all at once (the LDS store path takes 13 cycles per wave-instruction).
    amp_t x[IPT][kPartRows];
    u32x8 off[IPT];
    u32x16 c0, c1, c2, c3; // IPT == 1: the first coefficient batch travels with the offsets
    u32x8 rowoff1;         // ... and the row offsets as well: a class is written as soon as it is multiplied
#pragma unroll
    for (int i = 0; i < IPT; i++) {
        const bool live = FULL || tid + i * THREADS < ITEMS;
        off[i] = sload8<0>(rec[i]);
        if constexpr (IPT == 1) rowoff1 = sload8<32>(rec[i]);
        if constexpr (IPT == 1) {
            c0 = sload16<kRecCoefByte>(rec[i]); c1 = sload16<kRecCoefByte + 64>(rec[i]);
            if constexpr (T != 1) { c2 = sload16<kRecCoefByte + 128>(rec[i]); c3 = sload16<kRecCoefByte + 192>(rec[i]); }
            if constexpr (T == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(off[i]), "+s"(rowoff1), "+s"(c0), "+s"(c1));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(off[i]), "+s"(rowoff1), "+s"(c0), "+s"(c1), "+s"(c2), "+s"(c3));
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(off[i]));
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (SKIPS && off[i][c * T] == kSkipClass) continue; // every row of the class is an identity row (wave-uniform)
            if (live) {
#pragma unroll
                for (int j = 0; j < T; j++) x[i][c * T + j] = lds_load(base[i] ^ off[i][c * T + j]); // the class's T operands, read once
            }
        }
    }
    if (mid_barrier) __syncthreads(); // lanes of other waves write slots this one reads: every lane has its operands
    // Phase 2 per item: multiply-adds (T = 4: class 0, the second coefficient batch into the same registers, class 1), then
    // the item's 8 writes.
#pragma unroll
    for (int i = 0; i < IPT; i++) {
        const bool live = FULL || tid + i * THREADS < ITEMS;
        amp_t y[kPartRows];
        u32x8 rowoff;
        auto row = [&](int p, const coef_t *cf) { // y[p] = sum_j cf[j] * x[class of p][j]
            if (live) {
                const int q0 = (p / T) * T;
                amp_t acc = cmul(x[i][q0], cf[0]);
#pragma unroll
                for (int j = 1; j < T; j++) acc = cfma(x[i][q0 + j], cf[j], acc);
                y[p] = acc;
            }
        };
        if constexpr (T == 4) {
            // Every operand of the lane is in registers and the barrier is behind us: a class is written as soon as it is multiplied
            // (4 result registers live instead of 8 — the VGPRs that buys are the second tile of prefetch — and the LDS store path,
            // 13 cycles per wave-instruction, gets its work in two helpings)
            if constexpr (IPT != 1) {
                rowoff = sload8<32>(rec[i]);
                c0 = sload16<kRecCoefByte>(rec[i]); c1 = sload16<kRecCoefByte + 64>(rec[i]);
                c2 = sload16<kRecCoefByte + 128>(rec[i]); c3 = sload16<kRecCoefByte + 192>(rec[i]);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(rowoff), "+s"(c0), "+s"(c1), "+s"(c2), "+s"(c3));
            } else {
                rowoff = rowoff1;
            }
            if (!(SKIPS && off[i][0] == kSkipClass)) {
                const coef_t r0[4] = {sgpr_coef(c0, 0), sgpr_coef(c0, 1), sgpr_coef(c0, 2), sgpr_coef(c0, 3)};
                const coef_t r1[4] = {sgpr_coef(c1, 0), sgpr_coef(c1, 1), sgpr_coef(c1, 2), sgpr_coef(c1, 3)};
                const coef_t r2[4] = {sgpr_coef(c2, 0), sgpr_coef(c2, 1), sgpr_coef(c2, 2), sgpr_coef(c2, 3)};
                const coef_t r3[4] = {sgpr_coef(c3, 0), sgpr_coef(c3, 1), sgpr_coef(c3, 2), sgpr_coef(c3, 3)};
                row(0, r0); row(1, r1); row(2, r2); row(3, r3);
                if (live) asm volatile("" : "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3])); // class 0 is done before its registers are loaded over
            }
            const bool second = !(SKIPS && off[i][4] == kSkipClass);
            if (second) {
                c0 = sload16<kRecCoefByte + 256>(rec[i]); c1 = sload16<kRecCoefByte + 320>(rec[i]);
                c2 = sload16<kRecCoefByte + 384>(rec[i]); c3 = sload16<kRecCoefByte + 448>(rec[i]);
            }
            if (!(SKIPS && off[i][0] == kSkipClass) && live) { // class 0 leaves while class 1's coefficients arrive
#pragma unroll
                for (int p = 0; p < 4; p++) lds_put(base[i] ^ rowoff[p], y[p]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(c0), "+s"(c1), "+s"(c2), "+s"(c3));
            if (second) {
                const coef_t r0[4] = {sgpr_coef(c0, 0), sgpr_coef(c0, 1), sgpr_coef(c0, 2), sgpr_coef(c0, 3)};
                const coef_t r1[4] = {sgpr_coef(c1, 0), sgpr_coef(c1, 1), sgpr_coef(c1, 2), sgpr_coef(c1, 3)};
                const coef_t r2[4] = {sgpr_coef(c2, 0), sgpr_coef(c2, 1), sgpr_coef(c2, 2), sgpr_coef(c2, 3)};
                const coef_t r3[4] = {sgpr_coef(c3, 0), sgpr_coef(c3, 1), sgpr_coef(c3, 2), sgpr_coef(c3, 3)};
                row(4, r0); row(5, r1); row(6, r2); row(7, r3);
                if (live) {
#pragma unroll
                    for (int p = 4; p < 8; p++) lds_put(base[i] ^ rowoff[p], y[p]);
                }
            }
            continue; // (written above)
        } else if constexpr (T == 2) {
            if constexpr (IPT != 1) {
                rowoff = sload8<32>(rec[i]);
                c0 = sload16<kRecCoefByte>(rec[i]); c1 = sload16<kRecCoefByte + 64>(rec[i]);
                c2 = sload16<kRecCoefByte + 128>(rec[i]); c3 = sload16<kRecCoefByte + 192>(rec[i]); // two rows of two entries each
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(rowoff), "+s"(c0), "+s"(c1), "+s"(c2), "+s"(c3));
            } else {
                rowoff = rowoff1;
            }
            const u32x16 *cs[4] = {&c0, &c1, &c2, &c3};
#pragma unroll
            for (int c = 0; c < 4; c++) { // a class (two rows) is written as soon as it is multiplied
                if (SKIPS && off[i][c * 2] == kSkipClass) continue;
                const coef_t ra[2] = {sgpr_coef(*cs[c], 0), sgpr_coef(*cs[c], 1)}, rb[2] = {sgpr_coef(*cs[c], 2), sgpr_coef(*cs[c], 3)};
                row(2 * c, ra);
                row(2 * c + 1, rb);
                if (live) { lds_put(base[i] ^ rowoff[2 * c], y[2 * c]); lds_put(base[i] ^ rowoff[2 * c + 1], y[2 * c + 1]); }
            }
        } else {
            if constexpr (IPT != 1) {
                rowoff = sload8<32>(rec[i]);
                c0 = sload16<kRecCoefByte>(rec[i]); c1 = sload16<kRecCoefByte + 64>(rec[i]); // four rows of one entry each
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(rowoff), "+s"(c0), "+s"(c1));
            } else {
                rowoff = rowoff1;
            }
#pragma unroll
            for (int p = 0; p < kPartRows; p++) {
                if (SKIPS && off[i][p] == kSkipClass) continue;
                const coef_t r[1] = {sgpr_coef(p < 4 ? c0 : c1, p & 3)};
                row(p, r);
                if (live) lds_put(base[i] ^ rowoff[p], y[p]);
            }
        }
    }
}

// The pair / quad forms (TOP_G1, TOP_DIAG1, TOP_G2) for tiles of fewer than 2^3 amplitudes, where a block cannot be padded to
// three qubits: registers of one or two qubits.  One wave, a handful of amplitudes.
template <int B, int THREADS>
__device__ __forceinline__ void tile_op_small(amp_t *lds, ConstOps ops, int oi, uint32_t tid, int bank, const OpHeader h) {
    constexpr uint32_t E = 1u << B;
    const int kind = (int)(h[0] & 255u);
    ConstRec rec = &ops[oi].rec[bank][0];
    if (kind == TOP_G2) {
        if constexpr (B >= 2) {
            const uint32_t bl = h[2] & 255u, bh = (h[2] >> 8) & 255u;
            const uint32_t o1 = 1u << bl, o2 = 1u << bh, o3 = o1 | o2;
            if (tid < E / 4) {
                const uint32_t i00 = ins0(ins0(tid, ~(o1 - 1u)), ~(o2 - 1u));
                const amp_t x0 = lds[i00], x1 = lds[i00 | o1], x2 = lds[i00 | o2], x3 = lds[i00 | o3];
                amp_t y[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    amp_t acc = cmul(x0, rec_coef(rec, 4 * r));
                    acc = cfma(x1, rec_coef(rec, 4 * r + 1), acc);
                    acc = cfma(x2, rec_coef(rec, 4 * r + 2), acc);
                    acc = cfma(x3, rec_coef(rec, 4 * r + 3), acc);
                    y[r] = acc;
                }
                lds[i00] = y[0]; lds[i00 | o1] = y[1]; lds[i00 | o2] = y[2]; lds[i00 | o3] = y[3];
            }
        }
    } else if constexpr (B >= 1) { // TOP_G1 / TOP_DIAG1 (a diagonal is a 2x2 with two zeros here: these tiles are not a hot path)
        const uint32_t bh = h[2] & 255u, o1 = 1u << bh;
        if (tid < E / 2) {
            const uint32_t i0 = ins0(tid, ~(o1 - 1u));
            const amp_t a0 = lds[i0], a1 = lds[i0 | o1];
            if (kind == TOP_G1) {
                lds[i0] = cfma(a1, rec_coef(rec, 1), cmul(a0, rec_coef(rec, 0)));
                lds[i0 | o1] = cfma(a1, rec_coef(rec, 3), cmul(a0, rec_coef(rec, 2)));
            } else {
                lds[i0] = cmul(a0, rec_coef(rec, 0));
                lds[i0 | o1] = cmul(a1, rec_coef(rec, 1));
            }
        }
    }
}

// The blocks of one pass applied to the tile in LDS (tile buffer at LDS byte address lds_base = lds), a workgroup
// barrier after each.  The 16 header bytes of a block arrive with ONE s_load_dwordx4, fetched a block ahead.  Two ways of
// making the preparation of a block (bank, part record, group base: ~100 instructions) cheaper were built and measured on one
// box against this form, and neither paid: preparing the NEXT block in front of the barrier that ends the current one (the plan
// carried across the loop edge cost more scalar registers than the overlap won: 69.5 ms per step against 68.8), and a
// per-workgroup table in LDS of everything that does not depend on the tile (~40 instructions left: 67.4 against 67.2).
template <int B, int THREADS>
__device__ __forceinline__ void tile_apply_ops(amp_t *lds, uint32_t lds_base, ConstOps ops, int n_ops, uint32_t tid, uint64_t tile_base) {
    if constexpr (B < 3) {
        OpHeader hn = op_header(ops, 0);
        for (int oi = 0; oi < n_ops; oi++) {
            const OpHeader h = hn;
            hn = op_header(ops, oi + 1 < n_ops ? oi + 1 : oi);
            // Where the tile's bank is the identity (a CX whose control bit is 0 here) nothing happens at all.
            const int bank = op_bank(h, tile_base);
            if ((h[1] >> (16 + bank)) & 1u) continue;
            tile_op_small<B, THREADS>(lds, ops, oi, tid, bank, h);
            __syncthreads();
        }
    } else {
        OpHeader hn = op_header(ops, 0);
        for (int oi = 0; oi < n_ops; oi++) {
            const OpHeader h = hn;
            hn = op_header(ops, oi + 1 < n_ops ? oi + 1 : oi);
            const PartPlan<B, THREADS> cur = part_prepare<B, THREADS>(lds_base, ops, oi, h, tile_base, tid);
            const uint32_t info = cur.info;
            const bool mid = info & 16u;
            if (!(info & 1u)) continue; // the tile's bank is the identity (a CX whose control bit is 0 here): nothing happens at all
            switch (info & 14u) {
            case 4: tile_op_part<B, THREADS, 4, false>(cur, tid, mid); break;
            case 12: tile_op_part<B, THREADS, 4, true>(cur, tid, mid); break;
            case 2: tile_op_part<B, THREADS, 2, false>(cur, tid, mid); break;
            case 10: tile_op_part<B, THREADS, 2, true>(cur, tid, mid); break;
            case 0: tile_op_part<B, THREADS, 1, false>(cur, tid, mid); break;
            default: tile_op_part<B, THREADS, 1, true>(cur, tid, mid); break;
            }
            __syncthreads();
        }
    }
}

// B (tile size) and THREADS are compile-time so every per-thread loop has a static trip count: all LDS
// reads of an op are issued before its arithmetic, all writes after, and there is no loop bookkeeping.
// No run-time branch may skip the stage-out: on such a path the prefetch loads are the youngest vector-memory operations and
// the compiler waits for vmcnt(0) — the previous tile's stores — before every stage-in (0.2-0.7 % of a step in round 2).
// PACK: the pass also does the re-layout of the exchange that follows it (qsim_internal.h PackMap): every amplitude is stored
// at perm(its index) of `vout` instead of at its own index — the separate pack sweep over the shard (k_pack: one more read
// and write of the state per exchange) disappears.  perm is a permutation of index BITS, so it splits like the index itself
// into a per-lane part, a per-register part and a per-tile part, each permuted once; the stores keep their 128-byte runs
// unless one of the three lowest index bits leaves.
__device__ __forceinline__ uint64_t pack_perm(const PackMap &pm, uint64_t x) {
    uint64_t o = (x & pm.seg[0]) | ((x & pm.seg[1]) >> 1) | ((x & pm.seg[2]) >> 2) | ((x & pm.seg[3]) >> 3);
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (j < pm.k) o |= ((x >> pm.sel[j]) & 1ULL) << pm.to[j];
    return o;
}

// SPARSE: the variant for a pass over a partially written state (TileDev::zero_mask != 0, not generating).  Slots of a visited
// tile whose index has a zero_mask bit are zero by definition, and their loads are never issued: the engine puts the tile bits
// that are new to the support into the topmost register role, so the live slots of every lane are its first live_regs
// registers and the fetch is ONE wave-uniform choice between straight-line batches of APT, APT/2, APT/4 ... loads (a
// per-element "load or zero" select would make the compiler branch around each load and wait for vmcnt(0) per element, the
// previous tile's stores included).  New bits that are not there (more than the register role holds, a shuffled order, the low
// bits, tiles with tail guards) mask whole lanes off for the batch, or are loaded and zeroed as before: right, not fast, and only
// the sub-millisecond passes come that way.  Full sweeps run the SPARSE = false instantiation, which carries none of this.
template <int B, int THREADS, bool PACK = false, bool SPARSE = false>
__global__ __launch_bounds__(THREADS, QSIM_TILE_MIN_WAVES(THREADS)) void k_tile(amp_t *v, amp_t *vout, TileDev g, const TileOp *__restrict__ ops_g,
                                                  int n_ops, uint64_t ntiles, int tiles_per_wg, int n_scale, PackMap pm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    amp_t *lds = reinterpret_cast<amp_t *>(smem);
    constexpr uint32_t E = 1u << B;
    constexpr int APT = (E + THREADS - 1) / THREADS;                              // amplitudes per thread
    constexpr bool FULL = E / 4 >= THREADS && (E / 4) % THREADS == 0;              // no tail guards needed
    const int L = g.low_bits, H = g.n_high;
    uint64_t *hoff = reinterpret_cast<uint64_t *>(smem + (sizeof(amp_t) << B));
    ConstOps scales = (ConstOps)(uintptr_t)ops_g; // n_scale tile-uniform factors, then the n_ops blocks
    ConstOps ops = scales + n_scale;
    const uint32_t tid = threadIdx.x;
    // slot tid + k*THREADS swizzles to (sw(tid) ^ lds_sw_fold(k*THREADS >> kSwLow)) + k*THREADS: the swizzle is linear and the two
    // parts share no bit (tid < THREADS, a power of two >= 64)
    const uint32_t tid_sw = sw_slot(tid);
    auto stage_slot = [&](int k) { return (tid_sw ^ lds_sw_fold<kAmpShift>((uint32_t)(k * THREADS) >> kSwLow)) + (uint32_t)(k * THREADS); };
    const uint32_t lowmask = (1u << L) - 1u;
    const uint64_t nmask = g.n >= 64 ? ~0ULL : ((1ULL << g.n) - 1ULL);
    const uint64_t outer_mask = nmask & ~(g.high_mask | (uint64_t)lowmask) & ~g.zero_mask; // the tiles to visit: outer bits that may be 1

    // lds_load / lds_put address the tile by raw LDS byte address: that is only right while this kernel's dynamic
    // LDS region starts at 0, i.e. while nobody adds a static __shared__ array to it.  Fail loudly otherwise.
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();

    // global index offset of high-slot code j (bit i of j = tile-local bit L+i = global bit high[i])
    auto spread = [&](uint32_t j) {
        uint64_t out = 0;
        for (int i = 0; i < H; i++) out |= (uint64_t)((j >> i) & 1u) << g.high[i];
        return out;
    };
    for (uint32_t j = tid; j < (1u << H); j += THREADS) hoff[j] = spread(j);
    __syncthreads();

    // A workgroup walks `tiles_per_wg` consecutive tiles.  While tile j is being processed in LDS, the loads of
    // tile j+1 are already in flight into registers (APT amplitudes per lane), which keeps bytes in flight during
    // the op phase: the kernel is latency-bound (bandwidth follows the number of workgroups currently in their
    // memory phase), and LDS capacity caps the resident tiles at two per CU.
    // vmcnt counts loads and stores together, in issue order, and the compiler merges its counter state at the
    // loop head: the first iteration is peeled so that BOTH ways into the loop carry [prefetch loads][stores of
    // the previous tile] — the wait it inserts before the prefetched registers are used is then vmcnt(#stores),
    // i.e. exact, instead of draining the previous tile's stores as well.  The prefetch is skipped (wave-uniform
    // branch) when there is no next tile; an unconditional re-fetch there showed up as +6 % FETCH_SIZE, and peeling
    // the last iteration as well (four copies of the op code) overflowed the instruction cache: 11.2 vs 7.8 ms/pass.
    const uint64_t first_tile = (uint64_t)blockIdx.x * (uint64_t)tiles_per_wg;
    if (first_tile >= ntiles) return;
    const int cnt = (int)((ntiles - first_tile) < (uint64_t)tiles_per_wg ? (ntiles - first_tile) : (uint64_t)tiles_per_wg);

    // Element k of a lane is tile slot e = tid + k*THREADS.  With THREADS >= 2^L the run index e >> L splits without
    // carry into (tid >> L) + k*(THREADS >> L), and the bit deposit is linear over disjoint bits, so the global byte
    // offset of the element is  lane_off (per lane, once per workgroup)  +  k_off[k] (wave-uniform)  +  tile base.
    // Tiles of a workgroup are consecutive: the next base is a masked increment, not another bit deposit.
    // (the engine guarantees 2^L <= 64 <= THREADS)
    const uint64_t lane_off = (hoff[(tid >> L) & ((1u << H) - 1u)] | (uint64_t)(tid & lowmask)) << kAmpShift;
    uint64_t k_off[APT];
#pragma unroll
    for (int k = 0; k < APT; k++) k_off[k] = spread((uint32_t)(k * THREADS) >> L) << kAmpShift;
    auto elem_ptr = [&](uint64_t tile_base, int k) -> amp_t * {
        return reinterpret_cast<amp_t *>(reinterpret_cast<unsigned char *>(v) + ((tile_base << kAmpShift) + k_off[k]) + lane_off);
    };
    auto next_base = [&](uint64_t b) { return ((b | ~outer_mask) + 1ULL) & outer_mask; }; // +1 scattered over the outer bits

    // vout != v: the pass reads the state from one buffer and writes it to the other (the engine then swaps them).  Same
    // bytes, but the chip sustains more of them when a read stream and a write stream do not share addresses: the
    // n = 30 bench schedule with its blocks skipped 98.1 -> 93.3 ms, as it runs 107.7 -> 101.4 (profiles/r02).
    const int64_t out_shift = reinterpret_cast<unsigned char *>(vout) - reinterpret_cast<unsigned char *>(v); // wave-uniform
    uint64_t lane_out = 0, k_out[APT];
    if (PACK) {
        lane_out = pack_perm(pm, lane_off >> kAmpShift) << kAmpShift;
#pragma unroll
        for (int k = 0; k < APT; k++) k_out[k] = pack_perm(pm, k_off[k] >> kAmpShift) << kAmpShift;
    }
    amp_t pf[APT];
    const bool generate = g.from_zero_ket != 0; // wave-uniform
    // SPARSE: the lane's own index bits (lane and wave role, low bits) lie inside the support
    const bool sparse_lane_ok = !SPARSE || ((lane_off >> kAmpShift) & g.zero_mask) == 0;
    auto fetch = [&](uint64_t tb) {
        if (generate) { // |0...0>: amplitude 1 at global index 0 (tile base 0, slot 0), nothing to read
#pragma unroll
            for (int k = 0; k < APT; k++) pf[k] = amp_t{(real_t)((tb == 0 && k == 0 && tid == 0) ? g.amp0 : 0.0), (real_t)0};
            return;
        }
        if constexpr (SPARSE && FULL) {
            // exclusive branches, each a straight-line batch that writes every register exactly once (a register that one branch
            // loads and another one zeroes afterwards would have to wait for the load: vmcnt(0))
            auto batch = [&](auto live_c) {
                constexpr int LIVE = decltype(live_c)::value;
#pragma unroll
                for (int k = 0; k < APT; k++) pf[k] = k < LIVE ? *elem_ptr(tb, k) : amp_t{(real_t)0, (real_t)0};
            };
            const int live = g.live_regs; // wave-uniform
            if (!sparse_lane_ok) batch(std::integral_constant<int, 0>{}); // masked lanes generate no requests
            else if (APT >= 2 && live == APT / 2) batch(std::integral_constant<int, (APT >= 2 ? APT / 2 : APT)>{});
            else if (APT >= 4 && live == APT / 4) batch(std::integral_constant<int, (APT >= 4 ? APT / 4 : APT)>{});
            else if (APT >= 8 && live == APT / 8) batch(std::integral_constant<int, (APT >= 8 ? APT / 8 : APT)>{});
            else batch(std::integral_constant<int, APT>{});
            return;
        }
#pragma unroll
        for (int k = 0; k < APT; k++) {
            const uint32_t e = tid + k * THREADS;
            pf[k] = (FULL || e < E) ? *elem_ptr(tb, k) : amp_t{(real_t)0, (real_t)0};
        }
    };
    auto process = [&](uint64_t base, bool prefetch_next) {
        if (n_scale > 0) { // wave-uniform: blocks whose qubits all lie outside the tile are one factor per tile
            real_t fr = (real_t)1, fi = (real_t)0;
            for (int i = 0; i < n_scale; i++) {
                const int bank = op_bank(op_header(scales, i), base);
                const real_t cr = ((ConstCoef)scales[i].scale[bank])[0], ci = ((ConstCoef)scales[i].scale[bank])[1];
                const real_t nr = fr * cr - fi * ci;
                fi = fr * ci + fi * cr;
                fr = nr;
            }
#pragma unroll
            for (int k = 0; k < APT; k++) pf[k] = cmul(pf[k], make_coef(fr, fi));
        }
        if (SPARSE && !generate) { // slots outside the state's support are zero (not loaded, or unwritten memory the fallback loaded);
                                   // after the tile-uniform factors, so that they are +0 whatever the factors are
#pragma unroll
            for (int k = 0; k < APT; k++)
                if (!(sparse_lane_ok && ((k_off[k] >> kAmpShift) & g.zero_mask) == 0)) pf[k] = amp_t{(real_t)0, (real_t)0};
        }
#pragma unroll
        for (int k = 0; k < APT; k++) {
            const uint32_t e = tid + k * THREADS;
            if (FULL || e < E) lds[stage_slot(k)] = pf[k];
        }
        __syncthreads();
        if (prefetch_next) fetch(next_base(base));

        tile_apply_ops<B, THREADS>(lds, 0u, ops, n_ops, tid, base);

        // stage out: every LDS read first (one wait for all of them instead of one per pair of stores), then the stores,
        // whose wave-uniform address part (tile base + register-bit offset + distance to the output buffer) stays scalar
        amp_t so[APT];
#pragma unroll
        for (int k = 0; k < APT; k++) {
            const uint32_t e = tid + k * THREADS;
            if (FULL || e < E) so[k] = lds[stage_slot(k)];
        }
        if (PACK) {
            const uint64_t sbase = (pack_perm(pm, base) | pm.konst) << kAmpShift; // wave-uniform
#pragma unroll
            for (int k = 0; k < APT; k++) {
                const uint32_t e = tid + k * THREADS;
                if (FULL || e < E) *reinterpret_cast<amp_t *>(reinterpret_cast<unsigned char *>(vout) + lane_out + (sbase + k_out[k])) = so[k];
            }
        } else {
            const uint64_t sbase = (base << kAmpShift) + (uint64_t)out_shift; // wave-uniform
#pragma unroll
            for (int k = 0; k < APT; k++) {
                const uint32_t e = tid + k * THREADS;
                if (FULL || e < E) *reinterpret_cast<amp_t *>(reinterpret_cast<unsigned char *>(v) + lane_off + (sbase + k_off[k])) = so[k];
            }
        }
        __syncthreads();
    };

    uint64_t base = deposit(first_tile, outer_mask); // wave-uniform
    fetch(base);
    process(base, cnt > 1);                                                   // peeled first iteration
    for (int j = 1; j < cnt; j++) {                                           // steady state; the last one fetches nothing
        base = next_base(base);
        process(base, j + 1 < cnt);
    }
}

// ---------------------------------------------------------------------------------------------------
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

// Shard re-layout ahead of a global<->local qubit exchange: gathers so that the p selected index bits
// become the top p bits (the destination block id) while the other bits keep their order.  Writes are
// fully coalesced; reads come in runs of 2^bits[0] amplitudes.
// Scatter form: consecutive lanes READ consecutive amplitudes (always fully coalesced); a wave's 64 stores
// fall into 2^(selected bits below 6) contiguous segments, i.e. >= 128 B pieces for up to three selected
// bits wherever they are.  (The gather form would read 16/32-B fragments when bit 0 or 1 is selected and
// fetch those sectors once per destination block.)
// dst = (pext(src, sel) << rest_bits) | pext(src, keep).  PEXT over disjoint bit ranges splits, so the part
// that depends on the work tile is wave-uniform scalar work and the part that depends on the lane is
// computed once per thread, outside the tile loop.
__device__ __forceinline__ uint64_t extract(uint64_t x, uint64_t mask) { // software PEXT
    uint64_t out = 0;
    int k = 0;
    while (mask) {
        const uint64_t low = mask & (0 - mask);
        if (x & low) out |= 1ULL << k;
        k++;
        mask &= mask - 1;
    }
    return out;
}

// Block b of the packed layout need not follow block b-1 in memory: each of the 2^p blocks has its own destination, so
// a shard can write its blocks straight into the buffers of the group members that will own them (another shard's
// buffer on the same device, or a peer-mapped one) — pack and transfer in one kernel.  Up to 8 blocks (p <= 3) travel
// as kernel arguments; the single-buffer layout is the special case blk[b] = out + b * 2^(n-p).
struct PackDst { amp_t *blk[8]; };
__device__ __forceinline__ amp_t *pack_block(const PackDst &d, uint32_t b) {
    amp_t *r = d.blk[0];
#pragma unroll
    for (uint32_t j = 1; j < 8; j++) r = (b == j) ? d.blk[j] : r; // select chain: no runtime-indexed kernel-argument array
    return r;
}

template <int IPT, bool SPLIT>
__global__ __launch_bounds__(TPB) void k_pack(const amp_t *__restrict__ in, amp_t *__restrict__ out, PackDst dst, uint64_t N, int n,
                                              int p, uint64_t sel_mask, uint64_t ntiles, uint32_t skip, uint64_t zero_mask) {
    constexpr int SB = 10; // log2(TPB * IPT): index bits owned by the position inside a work tile
    static_assert(TPB * IPT == (1 << SB), "tile split");
    const int rest_bits = n - p;
    const uint64_t nmask = n >= 64 ? ~0ULL : ((1ULL << n) - 1ULL);
    const uint64_t keep_mask = nmask & ~sel_mask;
    const uint64_t lo = (1ULL << SB) - 1ULL;
    const uint64_t rest_mask = (1ULL << rest_bits) - 1ULL;
    const int pc_keep_lo = __popcll(keep_mask & lo), pc_sel_lo = __popcll(sel_mask & lo);
    uint64_t add[IPT];
#pragma unroll
    for (int k = 0; k < IPT; k++) {
        const uint64_t e = (uint64_t)k * TPB + threadIdx.x;
        add[k] = (extract(e, sel_mask & lo) << rest_bits) | extract(e, keep_mask & lo);
    }
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = ((extract(tile, sel_mask >> SB) << pc_sel_lo) << rest_bits) |
                              (extract(tile, keep_mask >> SB) << pc_keep_lo); // wave-uniform
        const uint64_t s0 = (tile << SB) + threadIdx.x;
        amp_t a[IPT];
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t sidx = s0 + (uint64_t)k * TPB;
            // zero_mask: index bits the state is zero in BY DEFINITION (memory outside its support was never written: qsim_state::support)
            a[k] = (sidx < N && !(sidx & zero_mask)) ? in[sidx] : amp_t{(real_t)0, (real_t)0};
        }
#pragma unroll
        for (int k = 0; k < IPT; k++) {
            const uint64_t sidx = s0 + (uint64_t)k * TPB;
            if (sidx >= N) continue;
            const uint64_t di = base | add[k];
            if (skip && ((skip >> (uint32_t)(di >> rest_bits)) & 1u)) continue; // a block nobody will read (its receiver holds nothing afterwards)
            if (SPLIT) pack_block(dst, (uint32_t)(di >> rest_bits))[di & rest_mask] = a[k];
            else out[di] = a[k];
        }
    }
}

// ===================================================================================================
// launchers
static inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
static inline unsigned grid_for(const LaunchCfg &cfg, uint64_t ntiles) {
    uint64_t g = ntiles;
    if (cfg.grid_cap > 0 && g > (uint64_t)cfg.grid_cap) g = (uint64_t)cfg.grid_cap;
    if (g > kMaxGrid) g = kMaxGrid;
    return (unsigned)(g ? g : 1);
}

hipError_t launch_init(const LaunchCfg &cfg, void *v, int n, double amp0) {
    const uint64_t N = 1ULL << n;
    uint64_t blocks = ceil_div(N, TPB);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(k_init, dim3((unsigned)blocks), dim3(TPB), 0, cfg.stream, (amp_t *)v, N, amp0);
    return hipGetLastError();
}

hipError_t launch_zero_outside(const LaunchCfg &cfg, void *v, int n, uint64_t zero_mask) {
    const uint64_t N = 1ULL << n;
    uint64_t grid = ceil_div(N, TPB);
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(k_zero_outside, dim3((unsigned)grid), dim3(TPB), 0, cfg.stream, (amp_t *)v, N, zero_mask);
    return hipGetLastError();
}

#define QSIM_DISPATCH_GUARD(KERN, IPT, items, ...)                                                                    \
    do {                                                                                                              \
        const uint64_t nt_ = ceil_div((items), (uint64_t)TPB * (IPT));                                                \
        if ((items) % ((uint64_t)TPB * (IPT)) == 0)                                                                   \
            hipLaunchKernelGGL((KERN<IPT, false>), dim3(grid_for(cfg, nt_)), dim3(TPB), 0, cfg.stream, __VA_ARGS__,    \
                               nt_);                                                                                  \
        else                                                                                                          \
            hipLaunchKernelGGL((KERN<IPT, true>), dim3(grid_for(cfg, nt_)), dim3(TPB), 0, cfg.stream, __VA_ARGS__,     \
                               nt_);                                                                                  \
    } while (0)

hipError_t launch_gate1(const LaunchCfg &cfg, void *v, int n, int q, const M2 &U) {
    const uint64_t N = 1ULL << n;
    if (q >= 6) {
        const uint64_t npairs = N >> 1;
        QSIM_DISPATCH_GUARD(k_gate1_hi, 4, npairs, (amp_t *)v, npairs, q, U);
    } else {
        QSIM_DISPATCH_GUARD(k_gate1_lo, 4, N, (amp_t *)v, N, q, U);
    }
    return hipGetLastError();
}

hipError_t launch_phase(const LaunchCfg &cfg, void *v, int n, int q, double lr, double li) {
    const uint64_t items = (1ULL << n) >> 1;
    QSIM_DISPATCH_GUARD(k_phase, 4, items, (amp_t *)v, items, q, lr, li);
    return hipGetLastError();
}

hipError_t launch_diag1_full(const LaunchCfg &cfg, void *v, int n, int q, double d0r, double d0i, double d1r,
                             double d1i) {
    const uint64_t N = 1ULL << n;
    QSIM_DISPATCH_GUARD(k_diag1_full, 4, N, (amp_t *)v, N, q, d0r, d0i, d1r, d1i);
    return hipGetLastError();
}

hipError_t launch_cx(const LaunchCfg &cfg, void *v, int n, int control, int target) {
    if (control == target) return hipSuccess; // quantum_simulator.c:99 — no index qualifies
    const uint64_t items = (1ULL << n) >> 2;
    const int lo = control < target ? control : target, hi = control < target ? target : control;
    const uint64_t cbit = 1ULL << control, tbit = 1ULL << target;
    QSIM_DISPATCH_GUARD(k_cx, 4, items, (amp_t *)v, items, lo, hi, cbit, tbit);
    return hipGetLastError();
}

hipError_t launch_gate2(const LaunchCfg &cfg, void *v, int n, int q_hi, int q_lo, const M4 &U) {
    const uint64_t items = (1ULL << n) >> 2;
    QSIM_DISPATCH_GUARD(k_gate2_hh, 2, items, (amp_t *)v, items, q_lo, q_hi, U);
    return hipGetLastError();
}

static int tile_lds_bytes(int tile_bits, int n_high) { return ((int)sizeof(amp_t) << tile_bits) + (8 << n_high); }

constexpr bool tile_has_pack(int b, int threads) { return kAmpShift == 4 && b == 12 && threads == 512; } // the production shape of fp64 shards

// How many registers of a lane hold slots inside the support (TileDev::live_regs): all of them, halved for every high bit in
// zero_mask counted from the top of the order down, as far as the register role reaches.  Tiles with tail guards: all.
static int tile_live_regs(const TileGeom &g, int threads, uint64_t zero_mask) {
    const int slots = 1 << g.tile_bits;
    if (slots / 4 < threads || (slots / 4) % threads != 0) return (slots + threads - 1) / threads; // not FULL: the guarded path loads every slot
    int live = slots / threads;
    for (int j = g.n_high - 1; j >= 0 && live > 1 && ((zero_mask >> g.high[j]) & 1ULL); j--) live >>= 1;
    return live;
}

template <int B, int THREADS>
static hipError_t launch_tile_t(const LaunchCfg &cfg, void *v, void *vout, const TileGeom &g, const TileOp *d_ops, int n_ops,
                                bool from_zero_ket, double amp0, uint64_t zero_mask, const PackMap *pack) {
    uint64_t tile_mask = (1ULL << g.low_bits) - 1ULL;
    for (int j = 0; j < g.n_high; j++) tile_mask |= 1ULL << g.high[j];
    const uint64_t nmask = g.n >= 64 ? ~0ULL : ((1ULL << g.n) - 1ULL);
    zero_mask &= nmask; // (a generating pass gets all bits from the engine: only the tile at base 0 exists)
    const uint64_t ntiles = 1ULL << __builtin_popcountll(nmask & ~tile_mask & ~zero_mask); // tiles whose base index may be non-zero
    const int lds = tile_lds_bytes(g.tile_bits, g.n_high);
    // the opt-in to more than 64 KiB of dynamic LDS is per device (a cluster drives several from one process)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    constexpr bool kHasPack = tile_has_pack(B, THREADS);
    const bool packed = pack != nullptr && pack->k > 0;
    if (packed && !kHasPack) return hipErrorNotSupported;
    // four instantiations at most (PACK x SPARSE), each opted in once per device
    const bool sparse = zero_mask != 0 && !from_zero_ket; // a pass over a partially written state: k_tile<SPARSE>
    static bool attr_set[4][64] = {{false}};
    auto opt_in = [&](const void *fn, int which) -> hipError_t {
        if (attr_set[which][dev]) return hipSuccess;
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess) attr_set[which][dev] = true;
        return e;
    };
    {
        hipError_t e = opt_in(reinterpret_cast<const void *>(&k_tile<B, THREADS, false, false>), 0);
        // (the warm-up call opts in both plain instantiations: a run from a reset needs the SPARSE one a pass or two later)
        if (e == hipSuccess && ((sparse && !packed) || cfg.warm_only)) e = opt_in(reinterpret_cast<const void *>(&k_tile<B, THREADS, false, true>), 1);
        if constexpr (kHasPack) {
            if (e == hipSuccess && packed)
                e = sparse ? opt_in(reinterpret_cast<const void *>(&k_tile<B, THREADS, true, true>), 3) : opt_in(reinterpret_cast<const void *>(&k_tile<B, THREADS, true, false>), 2);
        }
        if (e != hipSuccess) return e;
    }
    if (cfg.warm_only) return hipSuccess;
    TileDev td;
    td.tile_bits = g.tile_bits; td.low_bits = g.low_bits; td.n_high = g.n_high; td.n = g.n;
    td.from_zero_ket = from_zero_ket ? 1 : 0;
    td.amp0 = amp0;
    td.high_mask = 0;
    td.zero_mask = zero_mask;
    for (int j = 0; j < 16; j++) td.high[j] = 0;
    for (int j = 0; j < g.n_high; j++) { td.high_mask |= 1ULL << g.high[j]; td.high[j] = (int8_t)g.high[j]; }
    // the registers of a lane walk the topmost high bits (tile slot bits log2(THREADS) .. B-1): each of them, from the top, that
    // the state is zero in halves the registers that hold anything
    td.live_regs = tile_live_regs(g, THREADS, sparse ? zero_mask : 0);
    // tiles per workgroup: enough to amortise the exposed first load — 64 where that still leaves four rounds of workgroups
    // (2048), down to 8 otherwise.  Round 4, late: 64 instead of 8 takes 1 % off a step at every size (tools/tpw_sweep.py: n = 30
    // 66.0 -> 65.4 ms, 128 tiles 66.3, 256 68.3, one round of 512 workgroups 69.6; n = 28 17.14 -> 16.9 with 32; n = 32 260.7 -> 258.8) ...
    int tpw = cfg.grid_cap > 0 ? (int)((ntiles + cfg.grid_cap - 1) / (uint64_t)cfg.grid_cap) : 64;
    if (cfg.grid_cap <= 0)
        while (tpw > 8 && ntiles / (uint64_t)tpw < 2048) tpw >>= 1;
    // ... but never fewer workgroups than the chip holds at once (2 per CU with 64 KiB tiles): a workgroup that walks
    // several tiles prefetches the next one while it works, one with a single tile exposes its load.  Small registers
    // used to get one tile per workgroup (">= 4096 workgroups"): n = 24 356 k -> 502 k gate-applies/s, n = 25 229 k ->
    // 255 k, n = 26 129 k -> 133 k with the floor at 512; from n = 27 up there are 4096 workgroups of 8 tiles either way.
    constexpr uint64_t kMinWorkgroups = 512;
    while (tpw > 1 && ntiles / (uint64_t)tpw < kMinWorkgroups) tpw >>= 1;
    if (tpw < 1) tpw = 1;
    const uint64_t grid = (ntiles + tpw - 1) / (uint64_t)tpw;
    // d_ops: g.n_scale tile-uniform factors first, then the blocks
    const int n_scale = n_ops > 0 ? g.n_scale : 0;
    PackMap pm{};
#define QSIM_TILE_GO(PACK_, SPARSE_, PM_)                                                                                                          \
    hipLaunchKernelGGL((k_tile<B, THREADS, PACK_, SPARSE_>), dim3((unsigned)grid), dim3(THREADS), lds, cfg.stream, (amp_t *)v, (amp_t *)vout, td, d_ops, \
                       n_ops - n_scale, ntiles, tpw, n_scale, PM_)
    if constexpr (kHasPack) {
        if (packed) {
            if (sparse) QSIM_TILE_GO(true, true, *pack);
            else QSIM_TILE_GO(true, false, *pack);
            return hipGetLastError();
        }
    }
    if (sparse) QSIM_TILE_GO(false, true, pm);
    else QSIM_TILE_GO(false, false, pm);
#undef QSIM_TILE_GO
    return hipGetLastError();
}

// threads: 0 = the default for the tile size.  Tiles below 2^8 amplitudes (tiny registers) use the 2^8 kernel's
// tail guards with a smaller E, so every size from 1 to 13 bits has an instantiation.
// which (tile size, thread count) launch_tile picks for a geometry: the re-layout variant exists for one of them
static bool launch_tile_can_pack(const TileGeom &g, int threads) { return tile_has_pack(g.tile_bits, g.tile_bits == 12 && threads != 256 && threads != 1024 ? 512 : 0); }

hipError_t launch_tile(const LaunchCfg &cfg, void *v, void *vout, const TileGeom &g, const TileOp *d_ops, int n_ops, int threads,
                       bool from_zero_ket, double amp0, uint64_t zero_mask, const PackMap *pack) {
#define QSIM_TILE(B_, T_) launch_tile_t<B_, T_>(cfg, v, vout, g, d_ops, n_ops, from_zero_ket, amp0, zero_mask, pack)
    switch (g.tile_bits) {
    case 0: return QSIM_TILE(0, 64);
    case 1: return QSIM_TILE(1, 64);
    case 2: return QSIM_TILE(2, 64);
    case 3: return QSIM_TILE(3, 64);
    case 4: return QSIM_TILE(4, 64);
    case 5: return QSIM_TILE(5, 64);
    case 6: return QSIM_TILE(6, 64);
    case 7: return QSIM_TILE(7, 64);
    case 8: return QSIM_TILE(8, 64);
    case 9: return QSIM_TILE(9, 128);
    case 10: return threads == 512 ? QSIM_TILE(10, 512) : QSIM_TILE(10, 256);
    case 11: return threads == 512 ? QSIM_TILE(11, 512) : QSIM_TILE(11, 256);
    case 12:
        if (threads == 256) return QSIM_TILE(12, 256);
        if (threads == 1024) return QSIM_TILE(12, 1024);
        return QSIM_TILE(12, 512);
    case 13:
        // default: the shape with 64 KiB tiles runs 512 threads and two workgroups per CU (fp32); 128 KiB tiles take 1024
        if (threads == 512 || (threads == 0 && kAmpShift == 3)) return QSIM_TILE(13, 512);
        return QSIM_TILE(13, 1024);
#if QSIM_AMP_SHIFT == 3
    // unreachable (QSIM_OPT_TILE_BITS stops at 13: the op header packs only kLaneNibbles free tile bits), but without this instantiation
    // the compiler lays out the setup of f32 k_tile<13, 512> differently and the fp32 step is 1.2 % slower (DESIGN §3)
    case 14: return QSIM_TILE(14, 1024);
#endif
    default: return hipErrorInvalidValue;
    }
#undef QSIM_TILE
}

hipError_t launch_norm2(const LaunchCfg &cfg, const void *v, int n, double *d_out) {
    const uint64_t N = 1ULL << n;
    uint64_t blocks = ceil_div(N, (uint64_t)TPB * 8);
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_norm2, dim3((unsigned)blocks), dim3(TPB), 0, cfg.stream, (const amp_t *)v, N, d_out);
    return hipGetLastError();
}

hipError_t launch_block_prob(const LaunchCfg &cfg, const void *v, int n, int block_bits, double *d_out) {
    const uint64_t N = 1ULL << n;
    const uint64_t nblocks = (N + (1ULL << block_bits) - 1) >> block_bits;
    uint64_t grid = nblocks > 65536 ? 65536 : nblocks;
    hipLaunchKernelGGL(k_block_prob, dim3((unsigned)grid), dim3(TPB), 0, cfg.stream, (const amp_t *)v, N, block_bits, d_out,
                       nblocks);
    return hipGetLastError();
}

hipError_t launch_block_prob_masked(const LaunchCfg &cfg, const void *v, uint64_t hi_mask, uint64_t lo_mask, double *d_out) {
    const int lo_bits = __builtin_popcountll(lo_mask);
    const uint64_t nblocks = 1ULL << __builtin_popcountll(hi_mask);
    const uint64_t grid = nblocks > 65536 ? 65536 : nblocks;
    hipLaunchKernelGGL(k_block_prob_masked, dim3((unsigned)grid), dim3(TPB), 0, cfg.stream, (const amp_t *)v, hi_mask, lo_mask, lo_bits, d_out, nblocks);
    return hipGetLastError();
}

hipError_t launch_gather_masked(const LaunchCfg &cfg, const void *v, uint64_t base, uint64_t lo_mask, void *d_out) {
    const uint64_t count = 1ULL << __builtin_popcountll(lo_mask);
    uint64_t grid = ceil_div(count, TPB);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(k_gather_masked, dim3((unsigned)grid), dim3(TPB), 0, cfg.stream, (const amp_t *)v, base, lo_mask, count, (amp_t *)d_out);
    return hipGetLastError();
}

hipError_t launch_pack(const LaunchCfg &cfg, const void *in, void *out, void *const *blocks, int n, const int *bits, int p, uint32_t skip, uint64_t zero_mask) {
    uint64_t sel = 0;
    for (int j = 0; j < p; j++) sel |= 1ULL << bits[j];
    const uint64_t N = 1ULL << n;
    const uint64_t nt = ceil_div(N, (uint64_t)TPB * 4);
    unsigned grid = grid_for(cfg, nt);
    if (grid > 8192) grid = 8192; // persistent: the per-thread PEXT above is paid once per 2^10 * (nt / grid) amplitudes
    PackDst d{};
    if (blocks) {
        if (p > 3) return hipErrorInvalidValue;
        for (int b = 0; b < (1 << p); b++) d.blk[b] = (amp_t *)blocks[b];
        hipLaunchKernelGGL((k_pack<4, true>), dim3(grid), dim3(TPB), 0, cfg.stream, (const amp_t *)in, (amp_t *)nullptr, d, N, n, p, sel, nt, skip, zero_mask);
    } else {
        if (p > 5) skip = 0; // the mask has 32 bits
        hipLaunchKernelGGL((k_pack<4, false>), dim3(grid), dim3(TPB), 0, cfg.stream, (const amp_t *)in, (amp_t *)out, d, N, n, p, sel, nt, skip, zero_mask);
    }
    return hipGetLastError();
}
