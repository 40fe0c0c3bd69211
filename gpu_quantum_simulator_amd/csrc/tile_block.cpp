// tile_block.cpp — the blocks of a tile pass (scheduler.h TileBlock): their predicates, the row classes one LDS trip evaluates,
// the split of a fused op by a tile (to_block) and the sparse merging of a pass's neighbouring blocks (merge_blocks).  Pure host code.
#include "scheduler_impl.h"

namespace qsim {

using sched::is_zero;

int TileBlock::max_row_nnz() const {
    int best = 0;
    for (int v = 0; v < banks(); v++)
        for (int r = 0; r < dim(); r++) best = std::max(best, row(v, r).n);
    return best;
}

bool TileBlock::bank_is_identity(int v) const {
    for (int r = 0; r < dim(); r++)
        if (!row(v, r).is_identity_row(r)) return false;
    return true;
}

bool TileBlock::is_identity() const {
    for (int v = 0; v < banks(); v++)
        if (!bank_is_identity(v)) return false;
    return true;
}

void TileBlock::full_matrix(cd *out) const {
    const int d = dim(), D = d << ns;
    std::fill(out, out + (size_t)D * D, cd(0, 0));
    for (int v = 0; v < banks(); v++)
        for (int r = 0; r < d; r++)
            for (int j = 0; j < row(v, r).n; j++) out[(size_t)(v * d + r) * D + (v * d + row(v, r).col[j])] = row(v, r).val[j];
}

// ---- row classes ------------------------------------------------------------------------------------------------------------
namespace {

// The connected components of one bank's rows and columns (an entry joins its row and its column), numbered by their first
// row.  Fixed arrays, no heap: merge_blocks asks once per candidate merge, and the scheduler's host time hangs on it.
constexpr int kMaxDim = 1 << kMaxBlockQ;
struct Components {
    int n = 0;                                       // components that hold a row
    unsigned char of_row[kMaxDim], of_col[kMaxDim];  // component of each row / column
    unsigned char nrow[kMaxDim], ncol[kMaxDim];      // rows / columns of each component
    bool ident[kMaxDim];                             // every row of the component is a row of the identity
    int maxsz = 0;
    // false: a column nobody reads (not a unitary block), or a component that is not square or has more than kMaxRowNnz rows
    bool build(const TileBlock &b, int v) {
        const int D = b.dim();
        unsigned char parent[2 * kMaxDim], id[2 * kMaxDim]; // rows 0..D-1, columns D..2D-1
        for (int i = 0; i < 2 * D; i++) { parent[i] = (unsigned char)i; id[i] = 0xff; }
        auto find = [&](int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
        for (int r = 0; r < D; r++)
            for (int j = 0; j < b.row(v, r).n; j++) {
                const int a = find(r), c = find(D + b.row(v, r).col[j]);
                if (a != c) parent[a] = (unsigned char)c;
            }
        n = maxsz = 0;
        for (int r = 0; r < D; r++) {
            const int f = find(r);
            if (id[f] == 0xff) { id[f] = (unsigned char)n; nrow[n] = ncol[n] = 0; ident[n] = true; n++; }
            of_row[r] = id[f];
            nrow[id[f]]++;
            if (!b.row(v, r).is_identity_row(r)) ident[id[f]] = false;
        }
        for (int c = 0; c < D; c++) {
            const int f = find(D + c);
            if (id[f] == 0xff) return false;
            of_col[c] = id[f];
            ncol[id[f]]++;
        }
        for (int k = 0; k < n; k++) {
            if (nrow[k] != ncol[k] || nrow[k] > kMaxRowNnz) return false;
            maxsz = std::max(maxsz, (int)nrow[k]);
        }
        return true;
    }
};

inline int class_size(int maxsz) { return maxsz <= 1 ? 1 : maxsz <= 2 ? 2 : 4; }

} // namespace

bool TileBlock::classes(int &T, std::vector<std::vector<int>> &rows, std::vector<std::vector<int>> &cols) const {
    const int D = dim(), NB = banks();
    if (D > kMaxDim) return false;
    struct Comp { std::vector<int> r, c; bool ident; };
    std::vector<std::vector<Comp>> all((size_t)NB);
    int maxsz = 1;
    for (int v = 0; v < NB; v++) {
        Components cc;
        if (!cc.build(*this, v)) return false;
        maxsz = std::max(maxsz, cc.maxsz);
        std::vector<Comp> &cs = all[v];
        for (int k = 0; k < cc.n; k++) cs.push_back(Comp{{}, {}, cc.ident[k]});
        for (int r = 0; r < D; r++) cs[cc.of_row[r]].r.push_back(r);
        for (int c = 0; c < D; c++) cs[cc.of_col[c]].c.push_back(c);
    }
    T = class_size(maxsz);
    if (D % T) return false;
    rows.assign((size_t)NB, {});
    cols.assign((size_t)NB, {});
    for (int v = 0; v < NB; v++) {
        std::vector<Comp> &cs = all[v];
        // first-fit decreasing, identity components last so that they share classes with one another
        std::stable_sort(cs.begin(), cs.end(), [](const Comp &a, const Comp &b) {
            if (a.ident != b.ident) return !a.ident;
            return a.r.size() > b.r.size();
        });
        std::vector<std::vector<int>> br, bc; // bins
        for (const Comp &cp : cs) {
            size_t k = 0;
            while (k < br.size() && br[k].size() + cp.r.size() > (size_t)T) k++;
            if (k == br.size()) { br.emplace_back(); bc.emplace_back(); }
            br[k].insert(br[k].end(), cp.r.begin(), cp.r.end());
            bc[k].insert(bc[k].end(), cp.c.begin(), cp.c.end());
        }
        for (size_t k = 0; k < br.size(); k++) {
            if (br[k].size() != (size_t)T) return false; // a gap: cannot be laid out as whole classes
            rows[v].insert(rows[v].end(), br[k].begin(), br[k].end());
            cols[v].insert(cols[v].end(), bc[k].begin(), bc[k].end());
        }
    }
    return true;
}

bool TileBlock::classes_feasible() const {
    const int D = dim(), NB = banks();
    if (D > kMaxDim) return false;
    int maxsz = 1;
    int cnt[kMaxBanks][kMaxRowNnz + 1]; // components by size, per bank
    for (int v = 0; v < NB; v++) {
        Components cc;
        if (!cc.build(*this, v)) return false;
        maxsz = std::max(maxsz, cc.maxsz);
        for (int s = 0; s <= kMaxRowNnz; s++) cnt[v][s] = 0;
        for (int k = 0; k < cc.n; k++) cnt[v][cc.nrow[k]]++;
    }
    const int T = class_size(maxsz);
    if (D % T) return false;
    if (T < 4) return true; // sizes 1 and 2 always fill bins of 2 (D is even)
    for (int v = 0; v < NB; v++) { // bins of 4: every 3 takes a 1, an odd 2 takes two 1s, the rest fills up by itself
        const int ones = cnt[v][1] - cnt[v][3];
        if (ones < 0 || ones < 2 * (cnt[v][2] & 1)) return false;
    }
    return true;
}

// Splits a fused op (1 or 2 qubits at level 3) by the tile: qubits in `inside` stay matrix indices, the others become
// bank selectors.  The op must be block-diagonal in every qubit left outside.
TileBlock sched::to_block(const FusedOp &op, uint64_t inside) {
    TileBlock t;
    t.gates = op.gates;
    const int k = op.nq(), D = op.dim();
    const int qs[2] = {op.q_hi, op.q_lo};
    int in_pos[2], sel_pos[2]; // bit positions (in the op's row index) of the inside / outside qubits, most significant first
    for (int a = 0; a < k; a++) {
        const int pos = k - 1 - a;
        if (inside >> qs[a] & 1ULL) { in_pos[t.nq] = pos; t.q[t.nq++] = qs[a]; }
        else { sel_pos[t.ns] = pos; t.s[t.ns++] = qs[a]; }
    }
    const int d = 1 << t.nq;
    t.shape(t.nq, t.ns);
    auto compose = [&](int v, int r) { // op row index from bank index v and inside row index r
        int idx = 0;
        for (int a = 0; a < t.ns; a++) idx |= ((v >> (t.ns - 1 - a)) & 1) << sel_pos[a];
        for (int a = 0; a < t.nq; a++) idx |= ((r >> (t.nq - 1 - a)) & 1) << in_pos[a];
        return idx;
    };
    for (int v = 0; v < (1 << t.ns); v++)
        for (int r = 0; r < d; r++) {
            TileBlock::Row &row = t.row(v, r);
            for (int c = 0; c < d; c++) {
                const cd z = op.m[D * compose(v, r) + compose(v, c)];
                if (!is_zero(z)) { row.col[row.n] = (uint8_t)c; row.val[row.n++] = z; } // d <= 4 = kMaxRowNnz
            }
        }
    return t;
}

// ---- sparse merging inside a pass -------------------------------------------------------------------------
// Most fused clusters are permutations-times-phases or two independent 2x2 blocks (exact zeros), so the product
// of neighbours on a few tile qubits usually still has <= 4 entries per row.  Such a product costs ONE trip through
// LDS in k_tile instead of one per factor, which is what bounds a pass once it carries more than ~6 blocks.
// Order: a block may hop over earlier blocks it shares no TILE qubit with (they commute: outside the tile every block
// of the pass is block-diagonal); everything it shares a tile qubit with and cannot join blocks those qubits for the
// rest of the scan.  Selecting qubits are merged too: the product has one bank per value of the union (at most two).
namespace {

// Row `r` of bank `bv` of block `b`, embedded into the space of the tile qubits qs[0..k) (descending): the block acts
// on its own qubits and as the identity on the rest, so the row keeps its entries with the spectator bits copied.
struct Embedding {
    int pos[kMaxBlockQ]; // bit position (inside the k-bit index) of each of the block's qubits
    int mask = 0;
    Embedding(const TileBlock &b, const int *qs, int k) {
        for (int a = 0; a < b.nq; a++) {
            pos[a] = 0;
            for (int j = 0; j < k; j++)
                if (qs[j] == b.q[a]) pos[a] = k - 1 - j;
            mask |= 1 << pos[a];
        }
    }
    int sub(const TileBlock &b, int idx) const { // idx restricted to the block's qubits, most significant first
        int r = 0;
        for (int a = 0; a < b.nq; a++) r = (r << 1) | ((idx >> pos[a]) & 1);
        return r;
    }
    int spread(const TileBlock &b, int sub_idx) const {
        int r = 0;
        for (int a = 0; a < b.nq; a++) r |= ((sub_idx >> (b.nq - 1 - a)) & 1) << pos[a];
        return r;
    }
};

// the block's own bank index under the joint selector value v over ss[0..nss)
int own_bank(const TileBlock &b, const int *ss, int nss, int v) {
    int bv = 0;
    for (int a = 0; a < b.ns; a++)
        for (int j = 0; j < nss; j++)
            if (ss[j] == b.s[a]) bv |= ((v >> (nss - 1 - j)) & 1) << (b.ns - 1 - a);
    return bv;
}

} // namespace

void Scheduler::merge_blocks(std::vector<TileBlock> &blocks) const {
    const int kMaxQ = tile_.merge_max_q;
    constexpr int kMaxSel = 2;
    std::vector<int> rem(blocks.size()), next; // indices into `blocks`: the blocks themselves are moved, never copied
    for (size_t i = 0; i < blocks.size(); i++) rem[i] = (int)i;
    std::vector<TileBlock> out;
    TileBlock m;
    while (!rem.empty()) {
        TileBlock cur = std::move(blocks[(size_t)rem[0]]);
        uint64_t blocked = 0;
        next.clear();
        for (size_t i = 1; i < rem.size(); i++) {
            const TileBlock &op = blocks[(size_t)rem[i]];
            const uint64_t qm = op.in_mask();
            if (qm & blocked) { blocked |= qm; next.push_back(rem[i]); continue; }
            const uint64_t un = cur.in_mask() | qm, us = cur.sel_mask() | op.sel_mask();
            bool merged = false;
            if (__builtin_popcountll(un) <= kMaxQ && __builtin_popcountll(us) <= kMaxSel) {
                int qs[kMaxBlockQ], k = 0, ss[2], nss = 0;
                for (int b = 63; b >= 0; b--) {
                    if (un >> b & 1ULL) qs[k++] = b;
                    if (us >> b & 1ULL) ss[nss++] = b;
                }
                const int D = 1 << k;
                m = TileBlock();
                m.shape(k, nss);
                for (int a = 0; a < k; a++) m.q[a] = qs[a];
                for (int a = 0; a < nss; a++) m.s[a] = ss[a];
                m.gates = cur.gates + op.gates;
                const Embedding ea(cur, qs, k), eb(op, qs, k);
                bool fits = true;
                for (int v = 0; v < (1 << nss) && fits; v++) {
                    const int va = own_bank(cur, ss, nss, v), vb = own_bank(op, ss, nss, v);
                    for (int r = 0; r < D && fits; r++) { // row r of (op after cur) = sum_t op[r][t] * cur[t][.]
                        int cols[kMaxRowNnz * kMaxRowNnz], n = 0;
                        cd vals[kMaxRowNnz * kMaxRowNnz];
                        const TileBlock::Row &rb = op.row(vb, eb.sub(op, r));
                        for (int jb = 0; jb < rb.n; jb++) {
                            const int t = (r & ~eb.mask) | eb.spread(op, rb.col[jb]);
                            const TileBlock::Row &ra = cur.row(va, ea.sub(cur, t));
                            for (int ja = 0; ja < ra.n; ja++) {
                                const int c = (t & ~ea.mask) | ea.spread(cur, ra.col[ja]);
                                const cd z = rb.val[jb] * ra.val[ja];
                                int e = 0;
                                while (e < n && cols[e] != c) e++;
                                if (e == n) { cols[n] = c; vals[n++] = z; }
                                else vals[e] += z;
                            }
                        }
                        TileBlock::Row &row = m.row(v, r);
                        row.n = 0;
                        for (int e = 0; e < n; e++) {
                            if (is_zero(vals[e])) continue; // exact cancellation
                            // one LDS trip evaluates at most kMaxRowNnz entries per row — except on two qubits, where
                            // that is all four columns anyway
                            if (row.n == kMaxRowNnz) { fits = false; break; }
                            row.col[row.n] = (uint8_t)cols[e];
                            row.val[row.n++] = vals[e];
                        }
                    }
                }
                if (fits && k >= 2) fits = m.classes_feasible(); // one LDS trip evaluates whole row classes (TileBlock::classes)
                if (fits) {
                    for (int v = 0; v < (1 << nss); v++) // keep every row's entries in ascending column order
                        for (int r = 0; r < D; r++) {
                            TileBlock::Row &row = m.row(v, r);
                            for (int x = 1; x < row.n; x++)
                                for (int y = x; y > 0 && row.col[y - 1] > row.col[y]; y--) {
                                    std::swap(row.col[y - 1], row.col[y]);
                                    std::swap(row.val[y - 1], row.val[y]);
                                }
                        }
                    std::swap(cur, m);
                    merged = true;
                }
            }
            if (!merged) { blocked |= qm; next.push_back(rem[i]); }
        }
        if (!cur.is_identity()) out.push_back(std::move(cur));
        rem.swap(next);
    }
    blocks.swap(out);
}

} // namespace qsim
