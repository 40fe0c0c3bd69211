// pack_kernel.inc — the exchange re-layout as a sweep of its own (a tile pass can do it in its stores instead: k_tile PACK).

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
