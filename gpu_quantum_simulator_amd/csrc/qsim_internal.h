// qsim_internal.h — types shared by the engine (host C++) and the HIP kernels.  Not installed.
#ifndef QSIM_INTERNAL_H
#define QSIM_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/qsim.h"

namespace qsim {

// Row-major complex matrices passed BY VALUE as kernel arguments (they land in SGPRs / the scalar
// cache: the "constant memory" of quantum_simulator_preproces_constant.cu:58-61 without the 64 KiB cap).
struct M2 { double re[4], im[4]; };
struct M4 { double re[16], im[16]; };

// One fused block inside a cache-blocked pass = one trip of the tile through LDS.  Bit positions are TILE-LOCAL (see TileGeom).
//
//   TOP_PART   sparse 2^k x 2^k block on k = nq in {3..6} tile qubits, `terms` = T (1, 2 or 4) entries per row.  Per bank the
//              block is a direct sum of small dense matrices in a permuted basis (Scheduler / TileBlock::classes), so its rows
//              are laid out CLASS by class: T rows that read the same T operand slots — ONE LDS read per amplitude whatever T is.
//              The 2^k positions of a group are dealt in PARTS of 8 (8 / T whole classes); a lane owns one (group, part), the
//              parts of a group sit in different waves (part-major), so everything a wave needs of the block — operand offsets,
//              row offsets, coefficients — is ONE wave-uniform record (PartRec) read through scalar loads at immediate offsets
//              from one pointer:
//                  x[j]      = slot rec.off[c*T + j]                           (class c of the part, j < T)
//                  y[c*T+i]  = sum_j rec.coef[(c*T+i)*T + j] * x[j]            -> written to slot rec.rowoff[c*T+i]
//              Offsets are ready LDS byte offsets (layout swizzle applied).  A class whose T rows are all identity rows costs
//              nothing: off[c*T] = kSkipClass and rowoff[c*T .. c*T+T) = kSkipClass.  k > 3 needs a workgroup barrier between everybody's reads and the writes unless
//              every part writes exactly the slots it read (flags bit 1).
//              Blocks on fewer than three qubits are PADDED by the engine with tile bits they act on as the identity (same reads,
//              same multiply-adds, same writes per amplitude; one code path, one dispatch).
//              Most fused clusters of Clifford+T-like circuits are permutations times phases or two independent 2x2 blocks, and
//              so are products of neighbouring ones on a few qubits (Scheduler::merge_blocks).
//   TOP_SCALE  no qubit inside the tile: a factor per tile, applied while the tile is staged in (scale[bank]).
//   TOP_G1 / TOP_DIAG1 / TOP_G2   dense 2x2 / diagonal / dense 4x4 in pair and quad form: only in tiles of fewer than 2^3
//              amplitudes (registers of one or two qubits), which have no three bits to pad to; coefficients row-major in
//              rec[bank][0].coef as (re, im); TOP_DIAG1: rec[bank][0].off[0] = 1 when d0 == 1 (only the bit = 1 half moves).
// BANKS.  A block may also depend on up to two qubits OUTSIDE the tile, provided it is block-diagonal in them (a CX
// whose control is outside, any diagonal gate): such a qubit is constant over a tile, so it merely selects which
// 2^k x 2^k sub-block the tile gets.  nsel / selbit name those GLOBAL index bits; the bank index is
// bit(selbit[0]) or 2*bit(selbit[0]) + bit(selbit[1]) of the tile's base index, wave-uniform, and only that bank's
// records are ever loaded.  `ident` bit v: bank v is the identity — the block is skipped on those tiles.
enum : int32_t { TOP_G1 = 1, TOP_G2 = 2, TOP_DIAG1 = 3, TOP_PART = 4, TOP_SCALE = 5 };
constexpr int kMaxBanks = 4;
constexpr int kMaxOpQ = 6;                      // TOP_PART blocks span 3..6 tile qubits
constexpr int kPartRows = 8;                    // positions per part
constexpr int kMaxParts = 1 << (kMaxOpQ - 3);
constexpr uint32_t kSkipClass = 0xFFFFFFFFu;
constexpr uint32_t kOpFlagSkips = 1u, kOpFlagClosed = 2u;
struct PartRec {
    uint32_t off[kPartRows];      // operand j of class c at [c*T + j]
    uint32_t rowoff[kPartRows];   // position p writes slot rowoff[p]
    double coef[kPartRows * 4 * 2]; // entry j of position p: (re, im) at [(p*T + j)*2]; fp32 states: the float pairs (ur, ui), (-ui, ur) in the same 16 bytes
};
struct TileOp {
    // the first 16 bytes are fetched with ONE scalar load (s_load_dwordx4) a block ahead of their use and decoded with scalar
    // bit-field extracts
    uint8_t kind;         // dword 0
    uint8_t nq;           //   qubits of the block inside the tile (TOP_PART: 3..6 after padding)
    uint8_t terms;        //   TOP_PART: T = rows per class = entries per row (1, 2, 4), the same for every bank
    uint8_t nsel;         //   0..2 selecting qubits
    uint8_t selbit[2];    // dword 1: their global index bits, most significant bank bit first
    uint8_t ident;        //   bit v: bank v is the identity
    uint8_t flags;        //   kOpFlagSkips: some class is skipped; kOpFlagClosed: no barrier between reads and writes
    uint8_t b[8];         // dwords 2-3.  TOP_PART: nibble a of b[0..4] = the free tile-local bit that bit a of a lane's group index walks (kLaneNone: none; tile_op.cpp picks bank-conflict-free ones), b[7] = the kInfo* bits.  Pair / quad forms: b[0], b[1] = the block's tile-local bits, ascending
    uint32_t pad0[4];
    double scale[kMaxBanks][2]; // TOP_SCALE: the factor per bank as (re, im); fp32 states: two floats in the first 8 bytes
    uint32_t pad1[8];
    PartRec rec[kMaxBanks][kMaxParts];
};
// TOP_PART header packing (tile_op.cpp writes it, tile_kernel.inc part_geometry / part_prepare read it): kLaneNibbles lane
// nibbles in b[0..4], kLaneNone for a group-index bit that walks no tile bit, and in b[7] the bits of PartPlan::info the engine
// decides — log2 T at kInfoLog2TShift, kInfoSkips, kInfoBarrier (a workgroup barrier between the reads and the writes).
constexpr int kLaneNibbles = 10;
constexpr uint32_t kLaneNone = 15u;
constexpr int kInfoLog2TShift = 1;
constexpr uint32_t kInfoSkips = 8u, kInfoBarrier = 16u;
static_assert(sizeof(PartRec) == 64 + 512 && offsetof(TileOp, scale) == 32 && offsetof(TileOp, rec) == 128 &&
              sizeof(TileOp) == 128 + kMaxBanks * kMaxParts * sizeof(PartRec), "TileOp layout is shared with the device");

// Affine support (scheduler.h PassRegion).  A pass over a partially written state that knows the affine subspace the support lies
// in finds this record BEHIND its last block in the op buffer (it takes a TileOp's place there, read through scalar loads like
// the blocks): the tiles to visit are origin ^ span(gen[0 .. n_gen)), and an amplitude of the input is stale memory, staged in as
// zero, unless popcount(index & chk[j]) has parity bit j of chk_par for every j < n_chk.
constexpr int kAffineMaxGens = 18, kAffineMaxChecks = 18;
constexpr int kAffineWalk = 1, kAffineChecks = 2; // k_tile's `affine` argument: which halves of the record the pass goes by
struct TileAffine {
    uint32_t n_gen, n_chk, chk_par, pad0;
    uint64_t origin, pad1;
    uint64_t gen[kAffineMaxGens];
    uint64_t chk[kAffineMaxChecks];
};
static_assert(sizeof(TileAffine) <= sizeof(TileOp) && offsetof(TileAffine, gen) == 32, "TileAffine takes the place of a TileOp in the op buffer");

// LDS layout swizzle of a tile slot index: the 16-byte unit inside a 256-byte bank row (slot bits 0..3) is XORed with a
// linear image of the HIGHER slot bits.  A block on tile-local bits H ("holes") makes the lanes of a wave walk the
// lowest non-hole bits; a ds_read_b128 is conflict-free when, inside each of its four 16-lane groups (a 4-dimensional
// subspace of the five lowest lane bits, MI355X_MICROARCH.md LDS table), the lanes fall on 16 different units.
// Unswizzled, every hole among bits 0..3 halves the units touched.  Slot bit 4+j is given the column
//      j mod 5 == 0: 1111,   1: 0001,   2: 0010,   3: 0100,   4: 1000
// so that ANY five consecutive slot bits map to e0,e1,e2,e3,1111 — the largest set in GF(2)^4 of which every four
// are independent, and whose one dependency (all five) lies outside the lane groups' subspaces.  With holes the five
// lowest non-hole bits are not consecutive and some patterns still collide, but far fewer than with the first version
// of this swizzle (bit 4 only): modelled LDS cycles of the bench schedule's blocks 1.29x -> 1.17x the conflict-free
// count, and the same on other circuits (the blocks on 4 and 5 tile qubits punch many holes into the low bits).
// The map is linear over XOR: sw(a | b) = sw(a) ^ sw(b) for disjoint a, b, so per-thread bases are swizzled once and
// the wave-uniform operand offsets arrive pre-swizzled from the host (TileOp::off / rowoff, tile_op.cpp) —
// no extra instruction per access.
// fp32 amplitudes (8-byte slots): a ds_read_b64 serves 32 lanes per LDS cycle out of a 256-byte row = 32 units, so the unit is slot
// bits 0..4 and the columns live in GF(2)^5: slot bit 5+i (i < 5) gets e_i ^ e_(i+1 mod 5), slot bit 10+i the three ones 00111 << i —
// eight different vectors, none of them a unit vector, so that a block's free bits almost always contain five with independent images
// for the engine to hand to the five low lane bits (tile_op.cpp).  (Until late in round 4: slot bit 4 only, which left every
// higher bit without any image — 48 % of the fp32 kernel's LDS-active cycles were bank conflicts.)
// AMP_SHIFT = log2 of the slot size: 4 (fp64) or 3 (fp32).  The kernels (sw_slot, sw_byte, stage_slot) and the encoder call
// lds_sw_fold<AMP_SHIFT> directly: a forwarding wrapper in between changes the kernels' instruction schedule.
template <int AMP_SHIFT> constexpr int kLdsSwLow = AMP_SHIFT == 3 ? 5 : 4; // slot bits below this are the unit inside a bank row
template <int AMP_SHIFT>
__host__ __device__ __forceinline__ uint32_t lds_sw_fold(uint32_t hi) { // hi = slot >> kLdsSwLow (at most 10 bits)
    if (AMP_SHIFT == 3) {
        const uint32_t a = hi & 31u, b = (hi >> 5) & 7u;
        const uint32_t fa = a ^ (((a << 1) | (a >> 4)) & 31u);
        const uint32_t fb = ((0u - (b & 1u)) & 7u) ^ ((0u - ((b >> 1) & 1u)) & 14u) ^ ((0u - ((b >> 2) & 1u)) & 28u);
        return fa ^ fb;
    }
    const uint32_t f = (hi ^ (hi >> 5) ^ (hi >> 10)) & 31u;
    return ((f >> 1) & 15u) ^ ((0u - (f & 1u)) & 15u);
}

constexpr int kMaxTileHigh = 10; // high (non-contiguous) qubits per tile
struct TileGeom {
    int32_t tile_bits;          // B: log2 amplitudes per tile
    int32_t low_bits;           // L: tile-local bits [0,L) are global bits [0,L)
    int32_t n_high;             // B - L
    int32_t n;                  // qubits in this state (shard)
    int32_t high[kMaxTileHigh]; // global bit of tile-local bit L+j; any order (the scheduler emits ascending, the engine may reorder)
    int32_t n_scale;            // leading entries of the pass's op list that are TOP_SCALE factors, not blocks
};

// index bits [0, n) of a register of n qubits
inline uint64_t index_mask(int n) { return n >= 64 ? ~0ULL : ((1ULL << n) - 1ULL); }
// the global index bits a tile of geometry g holds
inline uint64_t tile_mask(const TileGeom &g) {
    uint64_t m = (1ULL << g.low_bits) - 1ULL;
    for (int j = 0; j < g.n_high; j++) m |= 1ULL << g.high[j];
    return m;
}

// Output permutation of a tile pass that also does the re-layout of an exchange (the pack): the amplitude read at index x is
// written at index  perm(x) = sum_i ((x & seg[i]) >> i)  |  sum_j (bit sel[j] of x) << to[j]  |  konst  of the OUTPUT buffer.
// sel[0..k) are the k <= 3 index bits that leave (ascending); the bits between them (seg[i]: the ones with i selected bits
// below them) close ranks.  One scratch buffer per shard: to[j] = n - k + j (the block index on top), konst = 0.  All shards
// of a cluster in one allocation: to[j] = the shard-id bit that takes the qubit, konst = the rest of the destination.
struct PackMap {
    uint64_t seg[4];
    uint64_t konst;
    int32_t sel[3], to[3];
    int32_t k; // 0: no re-layout
    // Deferred X gates (SchedConfig::defer_flips): the store goes to perm(x) ^ flip, a mask of OUTPUT index bits the caller sets.
    // perm(x) is the OR of a per-lane, a per-register and a per-tile part that share no output bit, so the launcher splits the
    // mask by which part owns each bit (flip_lane, flip_reg; the rest is the tile's) and the kernel XORs each piece once into
    // that part: nothing is added per amplitude.
    uint64_t flip, flip_lane, flip_reg;
};
// the identity permutation of n index bits: what a pass that only owes flips stores through
inline PackMap identity_pack_map() {
    PackMap pm{};
    pm.seg[0] = ~0ULL;
    return pm;
}

struct LaunchCfg {
    hipStream_t stream;
    int grid_cap; // 0 = one workgroup per work tile
    bool warm_only = false; // launch_tile: load the kernel's code object and set its attributes, launch nothing (the cold path does this while the state is being allocated)
};

// All launchers are asynchronous on cfg.stream and return the hipError_t of the launch.  `f32` selects the amplitude
// precision of the state `v` points to: false = fp64 complex (16 B per amplitude), true = fp32 complex (8 B).
hipError_t launch_init(const LaunchCfg &cfg, void *v, bool f32, int n, double amp0);
hipError_t launch_gate1(const LaunchCfg &cfg, void *v, bool f32, int n, int q, const M2 &U);
hipError_t launch_phase(const LaunchCfg &cfg, void *v, bool f32, int n, int q, double lr, double li);
hipError_t launch_diag1_full(const LaunchCfg &cfg, void *v, bool f32, int n, int q, double d0r, double d0i, double d1r, double d1i);
hipError_t launch_cx(const LaunchCfg &cfg, void *v, bool f32, int n, int control, int target);
hipError_t launch_gate2(const LaunchCfg &cfg, void *v, bool f32, int n, int q_hi, int q_lo, const M4 &U);
// from_zero_ket: the state is a not-yet-written basis state; the pass generates it in LDS instead of loading it
// zero_mask: index bits the state is known to be |0> in — tiles with such a bit in their base index are skipped, slots
// with one inside a tile are staged in as zero (their memory may never have been written)
// vout: where the pass writes the state — v itself (in place) or a second buffer of the same size
// pack (fp64, the default tile shape only — launch_tile_can_pack): vout is the output buffer of the re-layout, written at perm(index)
// affine (kAffineWalk | kAffineChecks; only with a zero_mask, never from_zero_ket): d_ops[n_ops] is a TileAffine the pass goes by;
// walk_gens: its n_gen, which the grid is sized by when the pass walks
hipError_t launch_tile(const LaunchCfg &cfg, void *v, void *vout, bool f32, const TileGeom &g, const TileOp *d_ops, int n_ops, int threads,
                       bool from_zero_ket, double amp0, uint64_t zero_mask = 0, const PackMap *pack = nullptr, int affine = 0, int walk_gens = 0);
bool launch_tile_can_pack(bool f32, const TileGeom &g, int threads);
// zeroes the amplitudes whose index has a bit of zero_mask set (the part of a state the tile passes have not written yet)
hipError_t launch_zero_outside(const LaunchCfg &cfg, void *v, bool f32, int n, uint64_t zero_mask);
hipError_t launch_norm2(const LaunchCfg &cfg, const void *v, bool f32, int n, double *d_out /* zeroed */);
// d_out[b] = sum of |a|^2 over amplitudes [b << block_bits, (b+1) << block_bits), fixed summation order
hipError_t launch_block_prob(const LaunchCfg &cfg, const void *v, bool f32, int n, int block_bits, double *d_out);
// d_out[w] = sum of |a|^2 over the amplitudes at deposit(w, hi_mask) | deposit(i, lo_mask), all i; 2^popcount(hi_mask) sums
hipError_t launch_block_prob_masked(const LaunchCfg &cfg, const void *v, bool f32, uint64_t hi_mask, uint64_t lo_mask, double *d_out);
// d_out[i] = v[base | deposit(i, lo_mask)], i < 2^popcount(lo_mask)
hipError_t launch_gather_masked(const LaunchCfg &cfg, const void *v, bool f32, uint64_t base, uint64_t lo_mask, void *d_out);
// out[dst] = in[src]: dst = (block << (n-p)) | rest, where block = the p bits of src at positions
// `bits` (ascending) and rest = the remaining n-p bits of src in order.
// `blocks` != NULL (p <= 3): block b goes to blocks[b] (2^(n-p) amplitudes each) instead of out + b * 2^(n-p).
// skip_blocks bit b: block b is not written (nobody will read it; with `blocks`, blocks[b] may then be NULL)
// zero_mask: index bits the source is zero in by definition (a partially written state): such amplitudes are packed as zeros, not loaded
hipError_t launch_pack(const LaunchCfg &cfg, const void *in, void *out, void *const *blocks, bool f32, int n, const int *bits, int p, uint32_t skip_blocks = 0,
                       uint64_t zero_mask = 0);

// ---- pauli.cpp: Pauli strings on one state that is shard `rank` of a register whose local qubits are the low qsim_num_qubits(s) bits
// of the masks (pauli_sweep.h has the sweeps themselves).  A partner is the buffer of shard rank ^ x_rank, quiescent, materialised
// and on the same device; it goes with x on rank qubits (x_rank != 0) and only with it, and then every local index is swept.
// The argument checks every Pauli entry point opens with, once its state or cluster is known to be there: no negative count, no
// NULL array (`third`: the one that goes with the masks — results, angles or coefficients), no mask bit at or above n, and
// `numbers` (angles or coefficients; `number` says which in the message) finite where there are any.  `report` is fail or cfail:
// whose last error it becomes.  `first`: the place of term 0 in the caller's own list, for the messages, when a part of a list is checked.
// Hidden: the library's exports stay what they were.
__attribute__((visibility("hidden"))) int check_pauli_terms(int (*report)(int, const char *, ...), const char *who, int n, const uint64_t *x_masks, const uint64_t *z_masks, const void *third,
                      const double *numbers, long num_terms, const char *number = "angle", long first = 0);
// <P_t> restricted to the shard; every term has the same x_rank.  Adds nothing up across shards.
int expect_paulis_shard(qsim_state *s, const void *partner, uint64_t rank, const uint64_t *x_masks, const uint64_t *z_masks, long num_terms,
                        double *out);
// How a list of rotations exp(-i theta/2 P) is carried out, in the caller's order.  A term that is X or Y on ONE qubit inside
// local_mask is a gate for the queue; every other term belongs to a run: a maximal stretch of consecutive such terms with equal x.
// c_masks (NULL: none): a term's control qubits.  The gate rule holds under at most ONE control (the 4x4); a run has one control mask.
struct RotRoute { long first, count; bool gate; };
std::vector<RotRoute> route_rotations(const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, uint64_t local_mask, const uint64_t *c_masks = nullptr);
long rotation_sweeps(long run_length); // ceil(run_length / K)
// One run; x carries the run's rank bits too.  Launches on the state's stream and returns.
int pauli_rot_run(qsim_state *s, void *partner, uint64_t rank, uint64_t x, const uint64_t *z_masks, const double *thetas, long count);
// The 2x2 of exp(-i theta/2 X) (y == false) or exp(-i theta/2 Y) as qsim_apply_1q takes it.
void pauli_rot_1q(bool y, double theta, double *U);
// dst = sum_t coeffs[t] Q_t |s->amps> for a settled state and checked arguments, on the state's stream: one out-of-place sweep per
// piece of an x group (qsim_pauli_sweeps counts them), the first stores, the others accumulate; num_terms == 0 writes zeros.  The
// gradient's lambda = H psi and the H of a Lanczos step (lanczos.cpp).
__attribute__((visibility("hidden"))) int pauli_sum_sweeps(qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, const double *coeffs, long num_terms, void *dst);

} // namespace qsim
#endif
