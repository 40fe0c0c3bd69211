// qft.h — what qft.hip (the kernel) and qft.cpp (the plan, the entry points) share: the quantum Fourier transform on any k qubits of
// the register, one sweep per DIGIT of at most ten bits.
//
// new[e | dep(y)] = 2^(-k/2) sum_x exp(+-2 pi i x y / 2^k) old[e | dep(x)] for every environment e; bit j of x and y is qubits[j].
// The register splits into digits d_1 ... d_m, s_p = d_1 + ... + d_(p-1).  Pass p works on the sub-register of register positions
// [s_p, k): its k_p = k - s_p bits hold (t, r), t the top d_p bits.  The pass replaces t by u = DFT over t (unitary scaling),
// multiplies by w^(+-r u), w = exp(2 pi i / 2^k_p), and stores the sub-register as r 2^d_p + u: the new digit goes to the low end and
// the rest moves up.  The last pass has no r: no twiddle, no move.  A pass that moves bits is not closed over its tile, so it reads
// one buffer and writes another.
//
// A TILE is the pass's digit and the lowest index bits outside it (pad_subset), B = min(qft_tile_bits, n) in all: permutation.h's
// tile, walked the same way (CtrlGeom / spread in their fp64 shape over amplitudes, in both precisions).  What the host hands the
// kernel is one record per pass: for every bit of a tile-local index where it lies in the buffer and in LDS — on the way in, where
// thread `tid` loads index j kTPB + tid, and on the way out, where it stores the output amplitude of that index in the ORDER OF THE
// OUTPUT ADDRESSES — and which bit of u or r it is.  Every map is linear over the bits of the index (OR for addresses, XOR for the
// swizzled LDS slots), so a thread forms its own part once and the part of j comes off scalar registers.
#ifndef QSIM_QFT_H
#define QSIM_QFT_H

#include "subset_sweep.h"

namespace qsim {

constexpr int kQftMaxDigitBits = 10;
// 64 KiB of amplitudes, permutation.h's sizes: 2^12 fp64 or 2^13 fp32 elements; a thread holds 16 or 32 of them, which is 4 or 5 bits
// of an LDS slot index: one ROUND of butterflies in registers between two LDS exchanges
constexpr int qft_tile_bits(bool f32) { return f32 ? 13 : 12; }
constexpr int qft_round_bits(bool f32) { return f32 ? 5 : 4; }
constexpr int kQftMaxTileBits = 13;
constexpr int kQftGridCap = 512; // as kPermGridCap; the resident grid is smaller (the kernel's registers let a CU hold one workgroup)
constexpr int kQftMaxPasses = 40; // a register has at most 40 qubits, a digit at least one bit

// LDS slot L of a tile: the digit value t on bits [0, d), the padding above.  The swizzle folds the slot's upper bit groups onto
// its lowest G bits (G = the round's): linear over XOR, a bijection, and the 2^G slots a thread holds in any round, like the slots
// of neighbouring lanes, fall on different bank groups.
constexpr uint32_t qft_swizzle(uint32_t slot, int G) { return slot ^ ((slot >> G) & ((1u << G) - 1u)) ^ (slot >> (2 * G)); }

// One pass, as the kernel gets it: through matrix.cpp's staging ring to the state's sweep scratch, read with scalar loads.  Bit i of
// a tile-local index in: the i-th lowest bit of in_mask; out: the i-th lowest bit of out_mask.  Bits from tile_bits up (a register smaller than a tile) have address 0 and are guarded.
struct QftPassRec {
    uint64_t in_addr[kQftMaxTileBits];   // 1 << qubit
    uint64_t out_addr[kQftMaxTileBits];
    uint64_t out_r[kQftMaxTileBits];     // the bit of r an output padding bit is (0: an environment bit or a bit of u)
    uint16_t in_lds[kQftMaxTileBits];    // qft_swizzle(1 << slot bit): a digit bit goes to slot bit m, padding above the digit
    uint16_t out_lds[kQftMaxTileBits];   // bit m of u is read from slot bit d - 1 - m: the butterflies leave X[u] at the bit-reversed slot
    uint16_t out_u[kQftMaxTileBits];     // the bit of u (0: a padding bit)
    uint8_t r_from[kQftMaxPasses], r_to[kQftMaxPasses]; // bit i of r: read at qubit r_from[i] of a tile's base, stored at qubit r_to[i]
    uint64_t sub_mask;                   // the sub-register's qubits
    int32_t d, kp, nr;                   // digit bits, sub-register bits, nr = kp - d bits of r
    uint32_t elems;                      // 2^tile_bits
    uint32_t inverse;
    double scale;                        // 2^(-d/2)
};
static_assert(sizeof(QftPassRec) <= 4096, "a record is a small operand of a staging slot");

struct QftPass {
    int d, kp, first;     // first = s_p: the sub-register is qubits[first .. k)
    bool oop;
    int tile_bits;
    uint64_t in_mask, out_mask;
};
struct QftPlan {
    int n, k, passes;
    bool f32;
    uint64_t tiles;       // per pass: 2^(n - tile_bits)
    uint64_t units;       // per pass, 16 bytes each, read and written once
    long trips_at_cap;
    int qubits[kQftMaxPasses];
    QftPass pass[kQftMaxPasses];
};
// The one rule.  false: k outside [0, n], n outside [0, 40], a qubit outside [0, n) or repeated, a NULL list with k > 0,
// max_digit_bits outside [0, 10] (0: the plan's own cap).
bool qft_plan(const int *qubits, int k, int n, bool f32, int max_digit_bits, QftPlan *out);
// the record of pass p of a plan
QftPassRec qft_pass_record(const QftPlan &plan, int p, bool inverse);

// src == dst: in place (the pass must move nothing).  rec: the record on the host, which is checked; d_rec: the same on the device.
// Reads 2^n amplitudes of src, writes 2^n of dst; asynchronous on cfg.stream.
hipError_t launch_qft_pass(const LaunchCfg &cfg, const void *src, void *dst, const QftPlan &plan, int p, const QftPassRec &rec, const QftPassRec *d_rec);

} // namespace qsim
#endif
