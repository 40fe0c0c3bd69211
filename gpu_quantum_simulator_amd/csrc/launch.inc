// launch.inc — the host launchers of every kernel above, one per entry of qsim_internal.h (kernels.hip picks the namespace).

static inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
// ceil(items / per_wg) workgroups, at most `cap` of them (the kernels stride over what is left) and at least one
static inline unsigned capped_grid(uint64_t items, uint64_t per_wg, uint64_t cap) {
    const uint64_t g = ceil_div(items, per_wg);
    return (unsigned)(g > cap ? cap : g ? g : 1);
}
static inline unsigned grid_for(const LaunchCfg &cfg, uint64_t ntiles) {
    return capped_grid(ntiles, 1, cfg.grid_cap > 0 && (uint64_t)cfg.grid_cap < kMaxGrid ? (uint64_t)cfg.grid_cap : kMaxGrid);
}

hipError_t launch_init(const LaunchCfg &cfg, void *v, int n, double amp0) {
    const uint64_t N = 1ULL << n;
    hipLaunchKernelGGL(k_init, dim3(capped_grid(N, TPB, 16384)), dim3(TPB), 0, cfg.stream, (amp_t *)v, N, amp0);
    return hipGetLastError();
}

hipError_t launch_zero_outside(const LaunchCfg &cfg, void *v, int n, uint64_t zero_mask) {
    const uint64_t N = 1ULL << n;
    hipLaunchKernelGGL(k_zero_outside, dim3(capped_grid(N, TPB, 16384)), dim3(TPB), 0, cfg.stream, (amp_t *)v, N, zero_mask);
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

// The one shape rule: the threads per workgroup a tile of 2^tile_bits slots runs with, given the caller's request (0 = the default
// for the size), in this namespace's precision.  Tiles below 2^8 amplitudes (tiny registers) use the 2^8 kernel's tail guards with
// a smaller E, so every size has a shape.  launch_tile instantiates exactly the (tile_bits, tile_threads) pairs this can return.
constexpr int tile_threads(int tile_bits, int threads) {
    if (tile_bits < 0) return 0;
    if (tile_bits <= 8) return 64;
    if (tile_bits == 9) return 128;
    if (tile_bits <= 11) return threads == 512 ? 512 : 256;
    if (tile_bits == 12) return threads == 256 || threads == 1024 ? threads : 512;
    // 13, default: the shape with 64 KiB tiles runs 512 threads and two workgroups per CU (fp32); 128 KiB tiles take 1024
    if (tile_bits == 13) return threads == 512 || (threads == 0 && kAmpShift == 3) ? 512 : 1024;
    return 1024;
}

constexpr bool tile_has_pack(int b, int threads) { return kAmpShift == 4 && b == 12 && threads == 512; } // the production shape of fp64 shards
// whether the shape launch_tile picks for a geometry has the re-layout variant
static bool launch_tile_can_pack(const TileGeom &g, int threads) { return tile_has_pack(g.tile_bits, tile_threads(g.tile_bits, threads)); }

// How many registers of a lane hold slots inside the support (TileDev::live_regs): all of them, halved for every high bit in
// zero_mask counted from the top of the order down, as far as the register role reaches.  Tiles with tail guards: all.
static int tile_live_regs(const TileGeom &g, int threads, uint64_t zero_mask) {
    const int slots = 1 << g.tile_bits;
    if (!tile_full(slots, threads)) return (slots + threads - 1) / threads; // the guarded path loads every slot
    int live = slots / threads;
    for (int j = g.n_high - 1; j >= 0 && live > 1 && ((zero_mask >> g.high[j]) & 1ULL); j--) live >>= 1;
    return live;
}

// PackMap::flip split by who owns each output bit: the lanes of a workgroup walk the low bits and the first log2(THREADS) - L
// high bits of the order, a lane's registers the rest of the tile, and perm carries each of those input bits to one output bit.
// (Only shapes without tail guards have the PACK variant: 2^L <= THREADS <= 2^B.)
static void split_flip(PackMap &pm, const TileGeom &g, int threads) {
    const int lane_high = __builtin_ctz((unsigned)threads) - g.low_bits; // high bits of the order that the lanes walk
    uint64_t lane_in = (1ULL << g.low_bits) - 1ULL, reg_in = 0;
    for (int j = 0; j < g.n_high; j++) (j < lane_high ? lane_in : reg_in) |= 1ULL << g.high[j];
    pm.flip_lane = pm.flip & pack_perm(pm, lane_in);
    pm.flip_reg = pm.flip & pack_perm(pm, reg_in);
}

template <int B, int THREADS>
static hipError_t launch_tile_t(const LaunchCfg &cfg, void *v, void *vout, const TileGeom &g, const TileOp *d_ops, int n_ops,
                                bool from_zero_ket, double amp0, uint64_t zero_mask, const PackMap *pack, int affine, int walk_gens) {
    zero_mask &= index_mask(g.n); // (a generating pass gets all bits from the engine: only the tile at base 0 exists)
    const bool sparse = zero_mask != 0 && !from_zero_ket; // a pass over a partially written state: k_tile<SPARSE>
    if (affine && (!sparse || walk_gens < 0 || walk_gens > kAffineMaxGens)) return hipErrorInvalidValue; // only SPARSE reads the record
    // tiles whose base index may be non-zero: the coordinate cube outside zero_mask, or the span of the record's generators
    const uint64_t ntiles = (affine & kAffineWalk) ? 1ULL << walk_gens : 1ULL << __builtin_popcountll(index_mask(g.n) & ~tile_mask(g) & ~zero_mask);
    const int lds = ((int)sizeof(amp_t) << g.tile_bits) + (8 << g.n_high); // the tile, then k_tile's hoff table
    constexpr bool kHasPack = tile_has_pack(B, THREADS);
    const bool packed = pack != nullptr && (pack->k > 0 || pack->flip != 0); // flips alone: the identity permutation (identity_pack_map)
    if (packed && !kHasPack) return hipErrorNotSupported;
    // four instantiations at most (PACK x SPARSE), all of one signature: the variant is chosen here, once, as an index and a pointer
    using TileKernel = void (*)(amp_t *, amp_t *, TileDev, const TileOp *, int, uint64_t, int, int, PackMap, int);
    const TileKernel plain[2] = {k_tile<B, THREADS, false, false>, k_tile<B, THREADS, false, true>};
    int which = sparse ? 1 : 0;
    TileKernel fn = plain[which];
    if constexpr (kHasPack) { // (what keeps the PACK instantiations from existing for other shapes)
        if (packed) {
            which += 2;
            fn = sparse ? k_tile<B, THREADS, true, true> : k_tile<B, THREADS, true, false>;
        }
    }
    // the opt-in to more than 64 KiB of dynamic LDS is per variant and per device (a cluster drives several from one process)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    static bool attr_set[4][64] = {{false}};
    auto opt_in = [&](TileKernel k, int idx) -> hipError_t {
        const hipError_t e = attr_set[idx][dev] ? hipSuccess : hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set[idx][dev] = e == hipSuccess;
        return e;
    };
    hipError_t e = opt_in(fn, which);
    // (the warm-up call opts in both plain instantiations: a run from a reset needs the SPARSE one a pass or two later)
    for (int i = 0; i < 2 && e == hipSuccess && cfg.warm_only; i++) e = opt_in(plain[i], i);
    if (e != hipSuccess || cfg.warm_only) return e;
    // the registers of a lane walk the topmost high bits (tile slot bits log2(THREADS) .. B-1): each of them, from the top, that
    // the state is zero in halves the registers that hold anything
    const TileDev td = make_tile_dev(g, from_zero_ket, amp0, zero_mask, tile_live_regs(g, THREADS, sparse ? zero_mask : 0));
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
    PackMap pm = packed ? *pack : PackMap{};
    if (pm.flip) {
        if ((pm.flip & ~index_mask(g.n)) != 0 || v == vout) return hipErrorInvalidValue; // a store outside the buffer / over amplitudes not read yet
        split_flip(pm, g, THREADS);
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(THREADS), lds, cfg.stream, (amp_t *)v, (amp_t *)vout, td, d_ops, n_ops - n_scale, ntiles, tpw,
                       n_scale, pm, affine);
    return hipGetLastError();
}

// threads: 0 = the default for the tile size (tile_threads).  One case per shape that exists.
hipError_t launch_tile(const LaunchCfg &cfg, void *v, void *vout, const TileGeom &g, const TileOp *d_ops, int n_ops, int threads,
                       bool from_zero_ket, double amp0, uint64_t zero_mask, const PackMap *pack, int affine, int walk_gens) {
#define QSIM_TILE(B_, T_) \
    case (B_) * 2048 + (T_): return launch_tile_t<B_, T_>(cfg, v, vout, g, d_ops, n_ops, from_zero_ket, amp0, zero_mask, pack, affine, walk_gens)
    switch (g.tile_bits * 2048 + tile_threads(g.tile_bits, threads)) {
    QSIM_TILE(0, 64);
    QSIM_TILE(1, 64);
    QSIM_TILE(2, 64);
    QSIM_TILE(3, 64);
    QSIM_TILE(4, 64);
    QSIM_TILE(5, 64);
    QSIM_TILE(6, 64);
    QSIM_TILE(7, 64);
    QSIM_TILE(8, 64);
    QSIM_TILE(9, 128);
    QSIM_TILE(10, 512);
    QSIM_TILE(10, 256);
    QSIM_TILE(11, 512);
    QSIM_TILE(11, 256);
    QSIM_TILE(12, 256);
    QSIM_TILE(12, 1024);
    QSIM_TILE(12, 512);
    QSIM_TILE(13, 512);
    QSIM_TILE(13, 1024);
#if QSIM_AMP_SHIFT == 3
    // unreachable (QSIM_OPT_TILE_BITS stops at 13: the op header packs only kLaneNibbles free tile bits), but without this instantiation
    // the compiler lays out the setup of f32 k_tile<13, 512> differently and the fp32 step is 1.2 % slower (DESIGN §3)
    QSIM_TILE(14, 1024);
#endif
    default: return hipErrorInvalidValue;
    }
#undef QSIM_TILE
}

hipError_t launch_norm2(const LaunchCfg &cfg, const void *v, int n, double *d_out) {
    const uint64_t N = 1ULL << n;
    hipLaunchKernelGGL(k_norm2, dim3(capped_grid(N, (uint64_t)TPB * 8, 4096)), dim3(TPB), 0, cfg.stream, (const amp_t *)v, N, d_out);
    return hipGetLastError();
}

hipError_t launch_block_prob(const LaunchCfg &cfg, const void *v, int n, int block_bits, double *d_out) {
    const uint64_t N = 1ULL << n;
    const uint64_t nblocks = (N + (1ULL << block_bits) - 1) >> block_bits;
    hipLaunchKernelGGL(k_block_prob, dim3(capped_grid(nblocks, 1, 65536)), dim3(TPB), 0, cfg.stream, (const amp_t *)v, N, block_bits, d_out,
                       nblocks);
    return hipGetLastError();
}

hipError_t launch_block_prob_masked(const LaunchCfg &cfg, const void *v, uint64_t hi_mask, uint64_t lo_mask, double *d_out) {
    const int lo_bits = __builtin_popcountll(lo_mask);
    const uint64_t nblocks = 1ULL << __builtin_popcountll(hi_mask);
    hipLaunchKernelGGL(k_block_prob_masked, dim3(capped_grid(nblocks, 1, 65536)), dim3(TPB), 0, cfg.stream, (const amp_t *)v, hi_mask, lo_mask, lo_bits, d_out, nblocks);
    return hipGetLastError();
}

hipError_t launch_gather_masked(const LaunchCfg &cfg, const void *v, uint64_t base, uint64_t lo_mask, void *d_out) {
    const uint64_t count = 1ULL << __builtin_popcountll(lo_mask);
    hipLaunchKernelGGL(k_gather_masked, dim3(capped_grid(count, TPB, 4096)), dim3(TPB), 0, cfg.stream, (const amp_t *)v, base, lo_mask, count, (amp_t *)d_out);
    return hipGetLastError();
}

hipError_t launch_pack(const LaunchCfg &cfg, const void *in, void *out, void *const *blocks, int n, const int *bits, int p, uint32_t skip, uint64_t zero_mask) {
    uint64_t sel = 0;
    for (int j = 0; j < p; j++) sel |= 1ULL << bits[j];
    const uint64_t N = 1ULL << n;
    const uint64_t nt = ceil_div(N, (uint64_t)TPB * 4);
    const unsigned grid = capped_grid(grid_for(cfg, nt), 1, 8192); // persistent: the per-thread PEXT above is paid once per 2^10 * (nt / grid) amplitudes
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
