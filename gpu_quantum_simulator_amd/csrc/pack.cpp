// pack.cpp — re-layouts of a state for an exchange and the buffer hand-overs that go with them: the pack kernel's entry points,
// qsim_flush_pack (the re-layout done by the last tile pass of the queue where it can be: flush_impl with a PackJob, engine.cpp)
// and qsim_swap_buffer / qsim_set_spare_buffer.  Calls settle / flush_impl / current_support and launch_pack; the routing of a
// flush's passes is engine.cpp's alone.
#include <cstdio>

#include "engine_state.h"

using namespace qsim;

// The index bits that leave in a re-layout: 1..most of them, ascending, inside the shard.
static int check_bits(const qsim_state *s, const char *who, const int *bits, int nbits, int most) {
    if (nbits < 1 || nbits > most || nbits > s->n) return fail(QSIM_ERR_ARG, "%s: %d bits unsupported", who, nbits);
    for (int j = 0; j < nbits; j++)
        if (bits[j] < 0 || bits[j] >= s->n || (j && bits[j] <= bits[j - 1])) return fail(QSIM_ERR_ARG, "%s: bit positions must be ascending and inside the shard", who);
    return QSIM_OK;
}

// keep_partial: a state that has only been written inside its support is packed as it is — amplitudes outside the support
// are packed as zeros without being loaded (k_pack zero_mask) — instead of having the zeros written out first.
static int pack_common(qsim_state *s, const int *bits, int nbits, void *dst, void *const *blocks, bool keep_partial, uint32_t skip_blocks) {
    if (!s || !bits || (!dst && !blocks)) return fail(QSIM_ERR_ARG, "NULL argument");
    QSIM_TRY(check_bits(s, "pack", bits, nbits, blocks ? 3 : 8));
    const size_t blk = (s->amp_bytes() << s->n) >> nbits;
    for (int b = 0; b < (blocks ? 1 << nbits : 0); b++) {
        if ((skip_blocks >> b) & 1u) continue;
        if (!blocks[b]) return fail(QSIM_ERR_ARG, "pack: destination block %d is NULL", b);
        const char *p = (const char *)blocks[b], *a = (const char *)s->amps;
        if (p < a + (s->amp_bytes() << s->n) && a < p + blk) return fail(QSIM_ERR_ARG, "pack: a destination block overlaps the state");
    }
    if (dst == s->amps) return fail(QSIM_ERR_ARG, "pack: dst must not alias the state");
    QSIM_TRY(settle(s, keep_partial));
    const bool as_is = s->partial; // (only keep_partial leaves it so)
    LaunchCfg cfg{s->stream, s->grid_cap};
    hipError_t e;
    {
        LaunchScope scope(s, QSIM_K_PACK);
        e = launch_pack(cfg, s->amps, dst, blocks, s->f32, s->n, bits, nbits, skip_blocks, as_is ? index_mask(s->n) & ~s->support : 0);
    }
    if (e != hipSuccess) return fail(QSIM_ERR_DEVICE, "pack launch failed: %s", hipGetErrorString(e));
    account(s, QSIM_K_PACK, 2.0 * (double)s->amp_bytes() * (double)(1ULL << s->n));
    return QSIM_OK;
}

extern "C" int qsim_pack_bits(qsim_state *s, const int *bits, int nbits, void *dst) { return pack_common(s, bits, nbits, dst, nullptr, false, 0); }
extern "C" int qsim_pack_bits_to(qsim_state *s, const int *bits, int nbits, void *const *dst_blocks) {
    return pack_common(s, bits, nbits, nullptr, dst_blocks, false, 0);
}
extern "C" int qsim_pack_bits_sparse(qsim_state *s, const int *bits, int nbits, void *dst, void *const *dst_blocks, uint32_t skip_blocks) {
    return pack_common(s, bits, nbits, dst_blocks ? nullptr : dst, dst_blocks, true, skip_blocks);
}

// qsim_flush + the re-layout of qsim_pack_bits_sparse in one call, so that the LAST tile pass of the queue can do the
// re-layout with its own stores (PackJob): no separate sweep over the state.  The output is one buffer in which source bit
// bits[j] lands on index bit to_bits[j] (NULL: n - nbits + j, the block index on top of a shard-sized buffer), the other
// bits close ranks below, and konst is ORed in (a cluster that keeps all its shards' buffers in one allocation addresses
// "block b of member j" that way).  Afterwards the state's own buffer holds stale data: the caller hands it its new contents
// (an exchange's receives, qsim_swap_buffer) and says what they are (qsim_set_support / qsim_reset_shard).
extern "C" int qsim_flush_pack(qsim_state *s, const int *bits, int nbits, const int *to_bits, uint64_t konst, void *out, uint64_t needed, uint32_t skip_blocks,
                               void **packed_at, int *fused) {
    if (!s || !bits) return fail(QSIM_ERR_ARG, "NULL argument");
    QSIM_TRY(check_bits(s, "flush_pack", bits, nbits, 8));
    if (nbits > 3 || s->f32) {
        // What a tile pass cannot re-lay-out (PackMap carries three selected bits, fp64): exchanges of 4..8 qubits — groups of 16
        // and more shards — and fp32 states take the plain route, flush then the pack kernel, with the same sparse roles (blocks
        // nobody reads are left out while the mask has a bit for each: k <= 5).  Only the one-buffer layout exists there.
        if (to_bits || konst) return fail(QSIM_ERR_ARG, "flush_pack: %d bits%s only into one buffer (no to_bits / konst)", nbits, s->f32 ? " of an fp32 state" : "");
        void *dst = out ? out : s->spare;
        if (!dst) return fail(QSIM_ERR_ARG, "flush_pack: no output buffer (lend one with qsim_set_spare_buffer)");
        QSIM_TRY(pack_common(s, bits, nbits, dst, nullptr, true, nbits <= 5 ? skip_blocks : 0));
        if (packed_at) *packed_at = dst;
        if (fused) *fused = 0;
        return QSIM_OK;
    }
    PackJob job;
    job.out = out;
    job.skip = skip_blocks;
    job.needed = needed;
    job.map.k = nbits;
    job.map.konst = konst;
    for (int j = 0; j < nbits; j++) {
        job.bits[j] = job.map.sel[j] = bits[j];
        job.map.to[j] = to_bits ? to_bits[j] : s->n - nbits + j;
        if (job.map.to[j] < s->n - nbits || job.map.to[j] > 62) return fail(QSIM_ERR_ARG, "flush_pack: destination bit %d collides with the bits that stay", job.map.to[j]);
    }
    const uint64_t nmask = index_mask(s->n);
    for (int i = 0; i <= nbits; i++) { // keep bits with i selected bits below them
        const uint64_t lo = i == 0 ? 0 : ((2ULL << bits[i - 1]) - 1ULL), hi = i == nbits ? nmask : ((1ULL << bits[i]) - 1ULL);
        job.map.seg[i] = hi & ~lo & nmask;
    }
    for (int i = nbits + 1; i < 4; i++) job.map.seg[i] = 0;
    if (!out && !s->spare) return fail(QSIM_ERR_ARG, "flush_pack: no output buffer (lend one with qsim_set_spare_buffer)");
    QSIM_TRY(flush_impl(s, &job));
    if (job.packed_at) {
        if (packed_at) *packed_at = job.packed_at;
        if (fused) *fused = 1;
        return QSIM_OK;
    }
    char *dst = (char *)(out ? out : s->spare);
    void *blocks[8];
    for (int b = 0; b < (1 << nbits); b++) {
        uint64_t at = konst;
        for (int j = 0; j < nbits; j++) at |= (uint64_t)((b >> j) & 1) << job.map.to[j];
        blocks[b] = dst + 16 * at;
    }
    if (trace_pack()) fprintf(stderr, "qsim: re-layout by the pack kernel (n = %d, support %llx)\n", s->n, (unsigned long long)current_support(s));
    QSIM_TRY(pack_common(s, bits, nbits, nullptr, blocks, true, skip_blocks));
    if (packed_at) *packed_at = dst;
    if (fused) *fused = 0;
    return QSIM_OK;
}

// Hands the state a different amplitude buffer and returns the old one: the second half of an exchange whose pack kernels
// wrote every shard's NEW contents into the group members' spare buffers.  Both buffers hold 2^n amplitudes on the
// state's device; whoever holds a buffer when it is destroyed frees it, so ownership simply travels with the pointers.
extern "C" int qsim_swap_buffer(qsim_state *s, void **buffer) {
    if (!s || !buffer || !*buffer) return fail(QSIM_ERR_ARG, "NULL argument");
    QSIM_TRY(qsim_flush(s));
    void *old = s->amps;
    s->amps = *buffer;
    *buffer = old;
    s->zero_ket_pending = false; // the new buffer's contents ARE the state: taken as written everywhere unless the caller says
    s->partial = false;          // otherwise (qsim_set_support, qsim_reset_shard)
    s->region_pending = false;
    if (s->spare == s->amps && !s->owns_spare) s->spare = old; // a lent spare that just became the state: the old state takes its place
    return QSIM_OK;
}

// Lends the state a second buffer of 2^n amplitudes on its device for out-of-place tile passes (QSIM_OPT_PINGPONG); the
// caller keeps ownership and may use the buffer itself whenever no gates are pending (after qsim_flush / qsim_sync the
// state is in its own buffer and the lent one holds garbage).  NULL takes it back.
extern "C" int qsim_set_spare_buffer(qsim_state *s, void *buffer) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    QSIM_TRY(qsim_flush(s));
    if (buffer == s->amps) return fail(QSIM_ERR_ARG, "set_spare_buffer: that is the state's own buffer");
    if (s->owns_spare && s->spare) {
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipStreamSynchronize(s->stream));
        (void)hipFree(s->spare);
    }
    s->spare = buffer;
    s->owns_spare = false;
    s->spare_failed = false;
    return QSIM_OK;
}
