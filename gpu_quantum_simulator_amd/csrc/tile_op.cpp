// tile_op.cpp — the TileOp encoder: a scheduled TileBlock as the record k_tile reads through scalar loads (layout:
// qsim_internal.h TileOp).  Host code with a bit-exact contract with tile_kernel.inc: the LDS offsets it stores are passed
// through the same swizzle (lds_sw_fold) and its header is decoded by part_geometry / part_prepare.
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "scheduler.h"

namespace qsim {

// tile-local bit of global qubit q under geometry g
static int local_bit(const TileGeom &g, int q) {
    if (q < g.low_bits) return q;
    for (int j = 0; j < g.n_high; j++)
        if (g.high[j] == q) return g.low_bits + j;
    return -1;
}

// S = log2 of the LDS slot size (4: fp64, 3: fp32).  The LDS byte offset of a tile slot as the kernel addresses it (sw_slot).
template <int S> static uint32_t slot_byte(uint32_t slot) { return (slot ^ lds_sw_fold<S>(slot >> kLdsSwLow<S>)) << S; }
// the unit bits of the swizzled slot 1 << b: which bank unit of a row the tile bit b moves a lane to
template <int S> static uint32_t unit_image(int b) { return b < kLdsSwLow<S> ? 1u << b : lds_sw_fold<S>(1u << (b - kLdsSwLow<S>)); }

static int rank_of(std::initializer_list<uint32_t> vs) { // rank of a few vectors of GF(2)^5
    uint32_t v[5] = {0, 0, 0, 0, 0};
    int n = 0, r = 0;
    for (uint32_t x : vs) v[n++] = x;
    for (int bit = 0; bit < 5; bit++) {
        int piv = -1;
        for (int i = r; i < n; i++)
            if (v[i] >> bit & 1u) { piv = i; break; }
        if (piv < 0) continue;
        std::swap(v[r], v[piv]);
        for (int i = 0; i < n; i++)
            if (i != r && (v[i] >> bit & 1u)) v[i] ^= v[r];
        r++;
    }
    return r;
}

// How well the free tile bits with unit images v[0..4], walked by lane bits l0..l4, spread a wave's LDS accesses over the banks
// (MI355X_MICROARCH.md, LDS): 0 = reads collide, 1 = reads conflict-free, 2 = reads and writes conflict-free.
//   fp64 (16-byte slots): a ds_read_b128 serves the 16 lanes of a 32-lane half with l2 ^ l3 ^ l4 = const in one cycle when they hit
//        16 different units of a 256-byte row — the images of l0, l1, l2 ^ l3, l2 ^ l4 independent; a ds_write_b128 the 8 lanes of
//        l0..l2 when theirs are independent modulo 8 units.
//   fp32 (8-byte slots): a ds_read_b64 serves the 32 lanes of a half when they hit 32 different units (the images of l0..l4
//        independent in GF(2)^5), a ds_write_b64 16 contiguous lanes out of a 128-byte row (l0..l3 independent modulo 16 units).
template <int S> static int lane_score(const uint32_t v[5]) {
    const bool reads = S == 4 ? rank_of({v[0], v[1], v[2] ^ v[3], v[2] ^ v[4]}) == 4 : rank_of({v[0], v[1], v[2], v[3], v[4]}) == 5;
    if (!reads) return 0;
    const bool writes = S == 4 ? rank_of({v[0] & 7u, v[1] & 7u, v[2] & 7u}) == 3 : rank_of({v[0] & 15u, v[1] & 15u, v[2] & 15u, v[3] & 15u}) == 4;
    return writes ? 2 : 1;
}

// Which free tile-local bit each bit of a lane's group index walks (tile_kernel.inc part_geometry).  Any assignment enumerates the
// groups; this one is chosen so that the lanes that share an LDS cycle fall on different banks.  The layout swizzle makes that true
// for holes-free low bits; a block's qubits punch holes, and the ascending assignment then collides for many hole patterns (24 % of
// the LDS-active cycles of the bench schedule were bank conflicts).  The five lowest lane bits get the first 5-tuple of distinct free
// bits, in lexicographic order, with the best lane_score; the rest of the free bits follow ascending.  No tuple with conflict-free
// reads: all ascending.
template <int S> static void order_lanes(const int *freeb, int nf, int *order) {
    for (int i = 0; i < nf; i++) order[i] = freeb[i];
    if (nf < 5) return;
    int t[5], best[5], best_score = 0;
    uint32_t img[16], v[5];
    for (int i = 0; i < nf; i++) img[i] = unit_image<S>(freeb[i]);
    auto search = [&](auto &&self, int depth, uint32_t taken) -> void {
        if (S == 3 && depth == 4 && rank_of({v[0], v[1], v[2], v[3]}) < 4) return; // fp32 reads need l0..l3 independent already
        if (depth == 5) {
            const int score = lane_score<S>(v);
            if (score > best_score) { best_score = score; std::copy(t, t + 5, best); }
            return;
        }
        for (int a = 0; a < nf && best_score < 2; a++) {
            if (taken >> a & 1u) continue;
            t[depth] = a;
            v[depth] = img[a];
            self(self, depth + 1, taken | 1u << a);
        }
    };
    search(search, 0, 0u);
    if (best_score == 0) return;
    bool taken[16] = {false};
    int n_o = 0;
    for (int i = 0; i < 5; i++) { order[n_o++] = freeb[best[i]]; taken[best[i]] = true; }
    for (int i = 0; i < nf; i++)
        if (!taken[i]) order[n_o++] = freeb[i];
}

bool to_tile_op(const TileGeom &g, const TileBlock &blk, TileOp &t, bool f32) {
    memset(&t, 0, sizeof t);
    const int k = blk.nq, NB = blk.banks();
    if (k > kMaxOpQ || blk.ns > 2) return false;
    t.nsel = blk.ns;
    for (int a = 0; a < blk.ns; a++) {
        if (local_bit(g, blk.s[a]) >= 0 || blk.s[a] < 0 || blk.s[a] >= g.n) return false; // selectors lie outside the tile
        t.selbit[a] = blk.s[a];
    }
    // qbit[a]: tile-local bit of the block's a-th qubit in ascending GLOBAL order = bit a of a row / column index (the pair / quad
    // forms of tiny tiles get the same bits sorted ascending in t.b[]; the two orders agree while TileGeom::high is ascending and
    // differ once the engine reorders the tile bits).
    int qbit[kMaxOpQ] = {0, 0, 0, 0, 0, 0};
    uint32_t used = 0;
    for (int a = 0; a < k; a++) {
        const int lb = local_bit(g, blk.q[k - 1 - a]);
        if (lb < 0) return false;
        qbit[a] = lb;
        used |= 1u << lb;
    }
    auto is1 = [&](const cd &z) { return z.real() == 1.0 && z.imag() == 0.0; };
    // a coefficient in the form the kernels read it: fp64 (re, im); fp32 the pairs (ur, ui), (-ui, ur) in the same 16 bytes
    auto put = [&](double *slot, const cd &z) {
        if (!f32) { slot[0] = z.real(); slot[1] = z.imag(); return; }
        const float r = (float)z.real(), i = (float)z.imag();
        const float four[4] = {r, i, -i, r};
        memcpy(slot, four, sizeof four);
    };
    for (int v = 0; v < NB; v++)
        if (blk.bank_is_identity(v)) t.ident |= 1 << v;
    if (k == 0) { // tile-uniform factor
        if (blk.ns == 0) return false;
        t.kind = TOP_SCALE;
        for (int v = 0; v < NB; v++) {
            const cd z = blk.at(v, 0, 0);
            if (f32) { const float two[2] = {(float)z.real(), (float)z.imag()}; memcpy(t.scale[v], two, sizeof two); }
            else { t.scale[v][0] = z.real(); t.scale[v][1] = z.imag(); }
        }
        return true;
    }
    const int maxnnz = blk.max_row_nnz();
    if (maxnnz > 4) return false;
    if (g.tile_bits < 3) { // a register of one or two qubits: no three tile bits to pad a block to, the pair / quad forms stay
        for (int a = 0; a < k; a++) t.b[a] = (uint8_t)qbit[a];
        std::sort(t.b, t.b + k);
        t.nq = k;
        if (k == 1) {
            bool diag = true;
            for (int v = 0; v < NB; v++) diag = diag && blk.at(v, 0, 1) == cd(0, 0) && blk.at(v, 1, 0) == cd(0, 0);
            t.kind = diag ? TOP_DIAG1 : TOP_G1;
            for (int v = 0; v < NB; v++) {
                if (diag) {
                    put(&t.rec[v][0].coef[0], blk.at(v, 0, 0));
                    put(&t.rec[v][0].coef[2], blk.at(v, 1, 1));
                    t.rec[v][0].off[0] = is1(blk.at(v, 0, 0)) ? 1 : 0;
                } else {
                    for (int e = 0; e < 4; e++) put(&t.rec[v][0].coef[2 * e], blk.at(v, e >> 1, e & 1));
                }
            }
            return true;
        }
        if (k != 2) return false;
        t.kind = TOP_G2; // the kernel's index bit 0 is t.b[0], bit 1 is t.b[1]: swap the qubits' roles if the tile order did
        const bool swapped = qbit[0] > qbit[1];
        auto sw = [&](int i) { return swapped ? ((i & 1) << 1) | (i >> 1) : i; };
        for (int v = 0; v < NB; v++)
            for (int e = 0; e < 16; e++) put(&t.rec[v][0].coef[2 * e], blk.at(v, sw(e >> 2), sw(e & 3)));
        return true;
    }
    // rows laid out class by class (TileBlock::classes): T rows that read the same T operand slots
    int T = 1;
    std::vector<std::vector<int>> crows, ccols;
    if (k == 1) { // classes() speaks about blocks on two and more qubits; a 2x2 is one class of two rows, or two of one
        bool diag = true;
        for (int v = 0; v < NB; v++) diag = diag && blk.at(v, 0, 1) == cd(0, 0) && blk.at(v, 1, 0) == cd(0, 0);
        T = diag ? 1 : 2;
        crows.assign((size_t)NB, {0, 1});
        ccols.assign((size_t)NB, {0, 1});
    } else if (!blk.classes(T, crows, ccols)) return false;
    // Fewer than three qubits: pad with tile bits the block does not touch (it acts on them as the identity).  Same LDS
    // reads, multiply-adds and writes per amplitude as the pair / quad forms had, through the one code path of the part form.
    int K = k;
    for (int lb = 0; K < 3 && lb < g.tile_bits; lb++)
        if (!(used >> lb & 1u)) { qbit[K++] = lb; used |= 1u << lb; }
    if (K < 3) return false;
    const int D = 1 << k, DK = 1 << K;
    t.kind = TOP_PART;
    t.nq = K;
    t.terms = T;
    {
        int freeb[16], order[16], nf = 0;
        for (int lb = 0; lb < g.tile_bits; lb++)
            if (!(used >> lb & 1u)) freeb[nf++] = lb;
        if (nf > kLaneNibbles) return false; // the header has no nibble for the bit a lane would have to walk
        if (f32) order_lanes<3>(freeb, nf, order);
        else order_lanes<4>(freeb, nf, order);
        uint64_t nib = 0;
        for (int a = 0; a < kLaneNibbles; a++) nib |= (uint64_t)(a < nf ? (uint32_t)order[a] : kLaneNone) << (4 * a);
        for (int a = 0; a < kLaneNibbles / 2; a++) t.b[a] = (uint8_t)(nib >> (8 * a));
    }
    // LDS BYTE offset of a slot code (bit a of the code sits at tile-local bit qbit[a]), already passed through the kernel's
    // layout swizzle (linear, so it commutes with the XOR the kernel combines it with)
    auto slot_off = [&](int code) {
        uint32_t o = 0;
        for (int a = 0; a < K; a++) o |= (uint32_t)((code >> a) & 1) << qbit[a];
        return f32 ? slot_byte<3>(o) : slot_byte<4>(o);
    };
    bool closed = true, skips = false;
    for (int v = 0; v < NB; v++)
        for (int p = 0; p < DK; p++) { // position p = copy (p / D) of the block over the padding bits, row crows[v][p % D] of it
            const int hi = (p / D) << k, r0 = crows[v][(size_t)(p % D)], r = hi | r0, c0 = ((p % D) / T) * T;
            PartRec &rec = t.rec[v][p / kPartRows];
            const int pp = p % kPartRows, cc = (pp / T) * T;
            rec.rowoff[pp] = slot_off(r);
            for (int j = 0; j < T; j++) {
                const int col = ccols[v][(size_t)(c0 + j)];
                rec.off[cc + j] = slot_off(hi | col); // the same list from every row of the class
                put(&rec.coef[(size_t)(pp * T + j) * 2], blk.at(v, r0, col)); // exact zero where the row does not use the column
            }
        }
    for (int v = 0; v < NB; v++)
        for (int part = 0; part < DK / kPartRows; part++) {
            PartRec &rec = t.rec[v][part];
            uint64_t reads = 0, writes = 0; // slot codes are < 64: compare the part's operand slots with the slots it writes
            for (int pp = 0; pp < kPartRows; pp++) {
                const int p = part * kPartRows + pp, hi = (p / D) << k;
                writes |= 1ULL << (hi | crows[v][(size_t)(p % D)]);
                reads |= 1ULL << (hi | ccols[v][(size_t)(p % D)]);
            }
            if (reads != writes) closed = false;
            for (int c = 0; c < kPartRows / T; c++) { // a class of identity rows only: nothing to do
                bool ident = true;
                for (int i = 0; i < T && ident; i++) {
                    const int p = part * kPartRows + c * T + i, r0 = crows[v][(size_t)(p % D)];
                    const TileBlock::Row &row = blk.row(v, r0);
                    ident = row.n == 1 && row.col[0] == r0 && is1(row.val[0]);
                }
                if (ident) { // the kernel asks off[] before its reads and rowoff[] before its writes
                    rec.off[c * T] = kSkipClass;
                    for (int i = 0; i < T; i++) rec.rowoff[c * T + i] = kSkipClass;
                    skips = true;
                }
            }
        }
    if (skips) t.flags |= kOpFlagSkips;
    if (closed) t.flags |= kOpFlagClosed;
    // what the kernel branches on, in the bit positions of tile_kernel.inc PartPlan::info
    const uint32_t log2T = T == 4 ? 2 : T == 2 ? 1 : 0;
    t.b[7] = (uint8_t)((log2T << kInfoLog2TShift) | (skips ? kInfoSkips : 0u) | (K > 3 && !closed ? kInfoBarrier : 0u));
    return true;
}

} // namespace qsim
