// support_tracker.cpp — SupportTracker (scheduler.h): the state's support as an affine subspace of GF(2)^n (affine.h), moved
// through the passes of a schedule; what each tile pass has to visit and may believe of its input follows from it (PassRegion).
// Pure host code.
#include "scheduler_impl.h"

namespace qsim {

void SupportTracker::start(int n, uint64_t initial_support) {
    n_ = n;
    const uint64_t nmask = index_mask(n);
    sup_ = initial_support & nmask;
    live_ = sup_ != nmask; // a dense state has nothing to refine
    V_ = AffineSpace::cube(sup_);
    wrote_.clear();
}

// V through one merged block.  The block acts on its tile qubits Q and is block-diagonal in its selectors S.  V's basis is split
// into vectors whose parts on Q | S are independent (at most |Q| + |S| <= 8: their 2^k combinations are the projections to
// enumerate) and vectors that are zero there, which pass through unchanged.
void SupportTracker::apply(const TileBlock &b) {
    if (b.nq == 0 || V_.dim() >= n_) return; // a factor per tile moves nothing; the whole space stays the whole space
    const uint64_t Q = b.in_mask(), QS = Q | b.sel_mask();
    std::vector<uint64_t> moving, fixed;
    for (uint64_t g : V_.basis.v) {
        for (uint64_t a : moving)
            if (((g ^ a) & QS) < (g & QS)) g ^= a;
        ((g & QS) ? moving : fixed).push_back(g);
    }
    auto gather = [](uint64_t x, const int *bits, int count) { // bits[0] is the most significant
        int out = 0;
        for (int a = 0; a < count; a++) out = 2 * out + (int)(x >> bits[a] & 1ULL);
        return out;
    };
    AffineSpace next;
    bool have = false;
    uint64_t x = V_.origin;
    for (uint64_t c = 0;; c++) { // Gray code over `moving`
        const int col = gather(x, b.q, b.nq), bank = gather(x, b.s, b.ns);
        for (int r = 0; r < b.dim(); r++) {
            const TileBlock::Row &row = b.row(bank, r);
            for (int j = 0; j < row.n; j++) {
                if (row.col[j] != col) continue;
                uint64_t y = x & ~Q;
                for (int a = 0; a < b.nq; a++) y |= (uint64_t)(r >> (b.nq - 1 - a) & 1) << b.q[a];
                if (!have) { next.origin = y; have = true; }
                else next.basis.insert(y ^ next.origin);
            }
        }
        if (c + 1 == (1ULL << moving.size())) break;
        x ^= moving[(size_t)__builtin_ctzll(c + 1)];
    }
    if (!have) return; // no entry at all in the columns V reaches: the state is zero from here on, and any V holds it
    for (uint64_t g : fixed) next.basis.insert(g);
    V_ = std::move(next);
}

void SupportTracker::visit(Pass &p) {
    if (!live_) return;
    if (p.kclass != QSIM_K_TILE) { live_ = false; return; } // the engine writes the zeros out in front of any other kernel: dense from here on
    const uint64_t nmask = index_mask(n_), tmask = tile_mask(p.geom) & nmask, outer = nmask & ~tmask;
    const uint64_t after = sup_ | tmask;
    PassRegion &r = p.region;
    r.on = true;
    r.support_before = sup_;
    r.checks = std::move(wrote_);
    wrote_.clear();
    const AffineSpace tiles = V_.project(outer);
    // the region this pass writes, as the next pass will test it; a bit outside `after` is in that pass's zero_mask already
    std::vector<ParityCheck> region;
    for (const ParityCheck &c : parity_checks(tiles, outer))
        if (!((c.mask & (c.mask - 1)) == 0 && c.parity == 0 && (c.mask & ~after))) region.push_back(c);
    const int cube_dim = __builtin_popcountll(outer & sup_);
    // (a pass that completes the support is followed by passes over a dense state, which test nothing: it writes the cube)
    r.refined = after != nmask && tiles.dim() < cube_dim && tiles.dim() <= kMaxRegionGens && (int)region.size() <= kMaxRegionChecks;
    if (r.refined) {
        r.origin = tiles.origin;
        r.gen = tiles.basis.v;
        wrote_ = std::move(region);
    } else { // the coordinate cube, as ever
        r.origin = 0;
        for (uint64_t m = outer & sup_; m; m &= m - 1) r.gen.push_back(m & (0 - m));
    }
    r.visited = 1.0 / (double)(1ULL << (__builtin_popcountll(outer) - (int)r.gen.size()));
    r.read_share = sup_ == 0 ? 0.0 : r.visited / (double)(1ULL << __builtin_popcountll(tmask & ~sup_));
    for (size_t k = (size_t)p.geom.n_scale; k < p.blocks.size(); k++) apply(p.blocks[k]);
    sup_ = after;
    if (sup_ == nmask) live_ = false; // dense from here on
}

} // namespace qsim
