// tile_kernel.inc — the cache-blocked pass: TileDev, the LDS swizzle and coefficient types, the hand-placed scalar loads, the part
// records and block forms, and k_tile itself.
//
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
static TileDev make_tile_dev(const TileGeom &g, bool from_zero_ket, double amp0, uint64_t zero_mask, int live_regs) {
    TileDev td{};
    td.tile_bits = g.tile_bits; td.low_bits = g.low_bits; td.n_high = g.n_high; td.n = g.n;
    td.from_zero_ket = from_zero_ket ? 1 : 0;
    td.amp0 = amp0;
    td.zero_mask = zero_mask;
    td.live_regs = live_regs;
    for (int j = 0; j < g.n_high; j++) { td.high_mask |= 1ULL << g.high[j]; td.high[j] = (int8_t)g.high[j]; }
    return td;
}

// `threads` lanes share `items` pieces of work in whole rounds: every lane has one in every round, no tail guard.
constexpr bool whole_rounds(uint32_t items, uint32_t threads) { return items >= threads && items % threads == 0; }
// A tile of `slots` amplitudes is staged in and out without tail guards (k_tile's FULL; tile_live_regs on the host): asked of
// the slot QUADS.  PartPlan::FULL asks the same of a block's 8-row items instead, and the two differ: 2^10 slots on 256
// threads are whole rounds of quads and half a round of items, so that tile stages unguarded and applies its blocks guarded.
constexpr bool tile_full(uint32_t slots, uint32_t threads) { return whole_rounds(slots / 4, threads); }

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
// The row offsets and the first NB coefficient batches of a record, and the wait that names them.  (The four coef_t of a batch
// stay written out where they are used: built by a helper, the same rows change the schedule of every k_tile with blocks.)
template <int NB>
__device__ __forceinline__ void load_rows(ConstRec rec, u32x8 &rowoff, u32x16 &c0, u32x16 &c1, u32x16 &c2, u32x16 &c3) {
    rowoff = sload8<32>(rec);
    c0 = sload16<kRecCoefByte>(rec); c1 = sload16<kRecCoefByte + 64>(rec);
    if constexpr (NB == 4) {
        c2 = sload16<kRecCoefByte + 128>(rec); c3 = sload16<kRecCoefByte + 192>(rec);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(rowoff), "+s"(c0), "+s"(c1), "+s"(c2), "+s"(c3));
    } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(rowoff), "+s"(c0), "+s"(c1));
    }
}

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
    static constexpr bool FULL = whole_rounds(ITEMS, THREADS); // over the items, not tile_full's slot quads
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
    constexpr uint32_t ITEMS = PartPlan<B, THREADS>::ITEMS;
    constexpr int IPT = PartPlan<B, THREADS>::IPT;
    constexpr bool FULL = PartPlan<B, THREADS>::FULL;
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
                load_rows<4>(rec[i], rowoff, c0, c1, c2, c3);
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
                load_rows<4>(rec[i], rowoff, c0, c1, c2, c3); // a batch: two rows of two entries each
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
                load_rows<2>(rec[i], rowoff, c0, c1, c2, c3); // a batch: four rows of one entry each
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
// Deferred X gates ride on the same stores (PackMap::flip): each part is XORed once with its share of the mask.  A flip of
// index bits 0..2 reverses 16-byte elements inside a 128-byte run; the run stays whole.
__host__ __device__ __forceinline__ uint64_t pack_perm(const PackMap &pm, uint64_t x) {
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
                                                  int n_ops, uint64_t ntiles, int tiles_per_wg, int n_scale, PackMap pm, int affine) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    amp_t *lds = reinterpret_cast<amp_t *>(smem);
    constexpr uint32_t E = 1u << B;
    constexpr int APT = (E + THREADS - 1) / THREADS;                              // amplitudes per thread
    constexpr bool FULL = tile_full(E, THREADS);                                   // no tail guards needed
    const int L = g.low_bits, H = g.n_high;
    uint64_t *hoff = reinterpret_cast<uint64_t *>(smem + (sizeof(amp_t) << B));
    ConstOps scales = (ConstOps)(uintptr_t)ops_g; // n_scale tile-uniform factors, then the n_ops blocks
    ConstOps ops = scales + n_scale;
    const uint32_t tid = threadIdx.x;
    // slot tid + k*THREADS swizzles to (sw(tid) ^ lds_sw_fold(k*THREADS >> kSwLow)) + k*THREADS: the swizzle is linear and the two
    // parts share no bit (tid < THREADS, a power of two >= 64)
    const uint32_t tid_sw = sw_slot(tid);
    auto stage_slot = [&](int k) { return (tid_sw ^ lds_sw_fold<kAmpShift>((uint32_t)(k * THREADS) >> kSwLow)) + (uint32_t)(k * THREADS); };
    auto live = [&](int k) { return FULL || tid + k * THREADS < E; }; // the lane's slot k exists (tiles with tail guards)
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
    // SPARSE with an affine record (qsim_internal.h TileAffine, behind the last block): the tiles are origin ^ span(gen), walked in
    // Gray-code order of the tile counter — the next base is ONE scalar XOR with gen[ctz(counter + 1)] — and a slot of the input
    // is stale unless every parity check holds.  Parity is linear and the index is lane part | register part | tile base over
    // disjoint bits, so bit j of (lane_par ^ k_par(k) ^ tile parities) is check j of the slot: one compare per register per tile.
    // The register part is linear in the bits of k as well: kb[i] is the vector of register 2^i, k_par(k) a few scalar XORs of them.
    typedef const __attribute__((address_space(4))) TileAffine *ConstAffine;
    ConstAffine aff = (ConstAffine)(ops + n_ops);
    const bool walk = SPARSE && (affine & kAffineWalk) != 0; // wave-uniform
    const int n_chk = SPARSE && (affine & kAffineChecks) ? (int)aff->n_chk : 0;
    uint64_t tcount = 0; // the tile counter of `base` (walk)
    constexpr int KB = APT > 1 ? __builtin_ctz((unsigned)APT) : 1; // (APT is a power of two)
    uint32_t lane_par = 0, kb[KB], chk_want = 0;
    if constexpr (SPARSE) {
#pragma unroll
        for (int i = 0; i < KB; i++) kb[i] = 0;
        if (n_chk > 0) chk_want = aff->chk_par;
        for (int j = 0; j < n_chk; j++) {
            const uint64_t m = aff->chk[j]; // wave-uniform
            lane_par |= (uint32_t)(__builtin_popcountll((lane_off >> kAmpShift) & m) & 1) << j;
#pragma unroll
            for (int i = 0; i < KB; i++)
                if ((1 << i) < APT) kb[i] |= (uint32_t)(__builtin_popcountll((k_off[(1 << i) < APT ? (1 << i) : 0] >> kAmpShift) & m) & 1) << j;
        }
    }
    auto k_par = [&](int k) { // wave-uniform
        uint32_t par = 0;
#pragma unroll
        for (int i = 0; i < KB; i++)
            if (k >> i & 1) par ^= kb[i];
        return par;
    };
    auto tile_par = [&](uint64_t b) { // the checks' parities of a tile base, against the wanted ones: 0 where the tile's share agrees
        uint32_t par = chk_want;
        for (int j = 0; j < n_chk; j++) par ^= (uint32_t)(__builtin_popcountll(b & aff->chk[j]) & 1) << j;
        return par;
    };
    auto next_base = [&](uint64_t b) -> uint64_t {
        if constexpr (SPARSE)
            if (walk) return b ^ aff->gen[__builtin_ctzll(tcount + 1ULL)];
        return ((b | ~outer_mask) + 1ULL) & outer_mask; // +1 scattered over the outer bits
    };

    // vout != v: the pass reads the state from one buffer and writes it to the other (the engine then swaps them).  Same
    // bytes, but the chip sustains more of them when a read stream and a write stream do not share addresses: the
    // n = 30 bench schedule with its blocks skipped 98.1 -> 93.3 ms, as it runs 107.7 -> 101.4 (profiles/r02).
    const int64_t out_shift = reinterpret_cast<unsigned char *>(vout) - reinterpret_cast<unsigned char *>(v); // wave-uniform
    uint64_t lane_out = 0, k_out[APT];
    if (PACK) {
        lane_out = pack_perm(pm, lane_off >> kAmpShift) << kAmpShift;
#pragma unroll
        for (int k = 0; k < APT; k++) k_out[k] = pack_perm(pm, k_off[k] >> kAmpShift) << kAmpShift;
        lane_out ^= pm.flip_lane << kAmpShift;
#pragma unroll
        for (int k = 0; k < APT; k++) k_out[k] ^= pm.flip_reg << kAmpShift; // wave-uniform
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
        for (int k = 0; k < APT; k++) pf[k] = live(k) ? *elem_ptr(tb, k) : amp_t{(real_t)0, (real_t)0};
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
        if constexpr (SPARSE) {
            if (!generate) { // slots outside the state's support are zero (not loaded, unwritten memory the fallback loaded, or memory outside
                             // the region the previous pass wrote); after the tile-uniform factors, so that they are +0 whatever the factors are
                const uint32_t tp = tile_par(base); // wave-uniform, and so is k_par(k) ^ tp: the lane's own vector is compared with a scalar
#pragma unroll
                for (int k = 0; k < APT; k++)
                    if (!(sparse_lane_ok && ((k_off[k] >> kAmpShift) & g.zero_mask) == 0 && lane_par == (k_par(k) ^ tp))) pf[k] = amp_t{(real_t)0, (real_t)0};
            }
        }
#pragma unroll
        for (int k = 0; k < APT; k++)
            if (live(k)) lds[stage_slot(k)] = pf[k];
        __syncthreads();
        if (prefetch_next) fetch(next_base(base));

        tile_apply_ops<B, THREADS>(lds, 0u, ops, n_ops, tid, base);

        // stage out: every LDS read first (one wait for all of them instead of one per pair of stores), then the stores,
        // whose wave-uniform address part (tile base + register-bit offset + distance to the output buffer) stays scalar
        amp_t so[APT];
#pragma unroll
        for (int k = 0; k < APT; k++)
            if (live(k)) so[k] = lds[stage_slot(k)];
        if (PACK) { // (two loops on purpose: one loop over a PACK ? : address leaves the guarded small tiles with other code)
            const uint64_t sbase = ((pack_perm(pm, base) | pm.konst) ^ (pm.flip & ~(pm.flip_lane | pm.flip_reg))) << kAmpShift; // wave-uniform
#pragma unroll
            for (int k = 0; k < APT; k++)
                if (live(k)) *reinterpret_cast<amp_t *>(reinterpret_cast<unsigned char *>(vout) + lane_out + (sbase + k_out[k])) = so[k];
        } else {
            const uint64_t sbase = (base << kAmpShift) + (uint64_t)out_shift; // wave-uniform
#pragma unroll
            for (int k = 0; k < APT; k++)
                if (live(k)) *reinterpret_cast<amp_t *>(reinterpret_cast<unsigned char *>(v) + lane_off + (sbase + k_off[k])) = so[k];
        }
        __syncthreads();
    };

    uint64_t base = deposit(first_tile, outer_mask); // wave-uniform
    if constexpr (SPARSE) {
        if (walk) { // the chunk's first base: the generators the Gray code of its first counter picks
            tcount = first_tile;
            base = aff->origin;
            const uint64_t gray = first_tile ^ (first_tile >> 1);
            const int n_gen = (int)aff->n_gen;
            for (int i = 0; i < n_gen; i++)
                if (gray >> i & 1ULL) base ^= aff->gen[i];
        }
    }
    fetch(base);
    process(base, cnt > 1);                                                   // peeled first iteration
    for (int j = 1; j < cnt; j++) {                                           // steady state; the last one fetches nothing
        base = next_base(base);
        if constexpr (SPARSE) tcount++;
        process(base, j + 1 < cnt);
    }
}
