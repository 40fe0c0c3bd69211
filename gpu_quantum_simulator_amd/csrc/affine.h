// affine.h — affine subspaces of GF(2)^n (n <= 64), index bits as coordinates: an origin and an XOR basis.  The scheduler
// tracks the state's support with one (support_tracker.cpp: a run from a reset stays inside o + span(g_1..g_d), and d grows by
// at most one per mixing gate, not by one per qubit touched).  Pure host code, no dependencies.
#ifndef QSIM_AFFINE_H
#define QSIM_AFFINE_H

#include <cstdint>
#include <vector>

namespace qsim {

// A linear subspace as an XOR basis: no two vectors share their highest bit, so reduce() brings any vector to its unique
// representative modulo the span (0 exactly for the members).
struct XorBasis {
    std::vector<uint64_t> v;
    int rank() const { return (int)v.size(); }
    uint64_t reduce(uint64_t x) const {
        for (uint64_t b : v)
            if ((x ^ b) < x) x ^= b;
        return x;
    }
    bool insert(uint64_t x) { // true: x was outside the span
        x = reduce(x);
        if (!x) return false;
        v.push_back(x);
        return true;
    }
    // Reduced row echelon form: every vector has a pivot bit (its highest) that no other vector has.
    void reduce_fully() {
        for (size_t i = 0; i < v.size(); i++)
            for (size_t j = 0; j < v.size(); j++)
                if (i != j && (v[j] >> (63 - __builtin_clzll(v[i])) & 1ULL)) v[j] ^= v[i];
    }
};

struct AffineSpace {
    uint64_t origin = 0;
    XorBasis basis;
    int dim() const { return basis.rank(); }
    // the coordinate cube over the bits of `mask`, origin 0
    static AffineSpace cube(uint64_t mask) {
        AffineSpace a;
        for (uint64_t m = mask; m; m &= m - 1) a.basis.v.push_back(m & (0 - m));
        return a;
    }
    // the image under x -> x & mask
    AffineSpace project(uint64_t mask) const {
        AffineSpace a;
        a.origin = origin & mask;
        for (uint64_t b : basis.v) a.basis.insert(b & mask);
        return a;
    }
};

// Parity checks (mask, parity) on index bits: x passes when popcount(x & mask) is odd exactly where parity says so.
struct ParityCheck {
    uint64_t mask;
    int parity;
};

// The set {x : (x & within) in a}, a inside the bits of `within`, as parity checks on those bits: one per bit of `within` that
// is no pivot of a's basis.  |within| - dim(a) checks.
inline std::vector<ParityCheck> parity_checks(const AffineSpace &a, uint64_t within) {
    XorBasis b = a.basis;
    b.reduce_fully();
    uint64_t pivots = 0;
    for (uint64_t g : b.v) pivots |= 1ULL << (63 - __builtin_clzll(g));
    std::vector<ParityCheck> out;
    for (uint64_t rest = within & ~pivots; rest; rest &= rest - 1) {
        const uint64_t f = rest & (0 - rest);
        uint64_t mask = f;
        for (uint64_t g : b.v)
            if (g & f) mask |= 1ULL << (63 - __builtin_clzll(g));
        out.push_back({mask, __builtin_parityll(a.origin & mask)});
    }
    return out;
}

} // namespace qsim
#endif
