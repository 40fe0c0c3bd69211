// pauli_sweep.h — how a Pauli sweep walks a state: what expect.hip (<psi|P|psi>, read-only), evolve.hip (exp(-i theta/2 P), in
// place), adjoint.hip (dE/dtheta: the backward sweep over psi and lambda, and lambda = H psi), crot.hip (the rotation under control
// qubits: CtrlGeom below), cadjoint.hip (the backward sweep under control qubits) and their host side pauli.cpp share.  DESIGN §7b
// opens with the same account.  combine.hip (linear combinations of whole states) is no Pauli sweep; it borrows the
// x == 0 geometry, the unit loads and the reducing grid; diagonal.hip (a real table over the whole register) borrows the
// unit type, the parity signs, rotate_diag, the resident and the reducing grid and has a geometry of its own (diagonal.h); sample.hip
// (shots drawn on the device) borrows the workgroup size and the resident grid and nothing else (sample.h); measure.hip
// (the weight of a measurement's outcome and the collapse onto it) borrows CtrlGeom and spread, with the outcome's bits as
// `ones`, the unit loads and the two grids (measure.h).
//
// A string is two masks: x (bit q: X or Y on qubit q) and z (bit q: Z or Y); s(j) = (-1)^popcount(j & z).  P maps every index
// pair {j, j ^ x} to itself, so a sweep visits one member j of each pair — the one with the highest bit h of x clear — and meets
// the other one as its partner; x == 0 visits every index and has no partner.  `full`: the pair's highest x bit selects the shard,
// so every index of buffer a is visited and its partner j ^ x lies in ANOTHER buffer b.  All strings of one sweep share x.
//
// Work is dealt in UNITS of 16 bytes per lane (one fp64 amplitude, two fp32 amplitudes), consecutive lanes on consecutive units;
// the partner unit (j ^ x) permutes the same 128-byte lines, so both streams stay coalesced for any x.  A unit index
// t = (q << kTidBits) | tid is expanded to an amplitude index by a bit insertion (the zero at bit h), which is linear over OR of
// disjoint bit sets: popcount(j & z) = popcount(E(q << kTidBits) & z) + popcount(E(tid) & z) (+ z bit 0 for the odd fp32 slot).
// The first part is uniform over the workgroup (scalar unit), the second is constant per thread.
// fp32 corners: x odd puts the partner in the other half of its unit; x == 1 on one state puts both members of a pair in ONE unit
// (odd_slot == 0: every unit is visited, its even slot is j); a register of one amplitude is 8 bytes long, no unit
// (load_unit_or_one; k_pauli_rot takes a single-thread path of its own).
//
// What the kernels share is here only where sharing left every kernel body instruction for instruction as it was.  Each kernel
// therefore still has its own: the way from units to (ar, ai, br, bi) with the fp32 half-swap in one line (shared, it changed the
// fp32 paired instantiations of k_expect and of k_pauli_adjoint), the thread's own parity mask `own` (k_pauli_rot, k_pauli_adjoint
// and k_pauli_sum changed), the choice "s ? odd_slot_sign : sg" (as a function of s it changed all four) and the block reduction of
// k_expect and k_pauli_adjoint (both changed).  The way back, own_unit and partner_unit, is shared.
//
// Grids.  Every workgroup of a sweep walks the same number of trips, so a second, partly filled round of workgroups would cost a
// whole round: the default grid is what is resident at once (resident_grid).  Two rules cap it, on purpose differently: reducing_grid
// (k_expect, k_pauli_adjoint) and writing_grid (k_pauli_rot, k_pauli_sum), which say why.
#ifndef QSIM_PAULI_SWEEP_H
#define QSIM_PAULI_SWEEP_H

#include <type_traits>

#include "qsim_internal.h"

namespace qsim {

// ---- sweep descriptors: what pauli.cpp hands to the launchers ---------------------------------------------------------------
constexpr int kMaxPauliTermsPerSweep = 32; // slots of the largest k_expect instantiation and term records of k_pauli_rot;
                                           // qsim_pauli_terms_per_sweep() / qsim_pauli_rotations_per_sweep() is what a call uses
struct PauliSweep {
    uint64_t x;
    bool full;
    int count;      // strings, all with this x; a rotation sweep applies them in order
    uint64_t z[kMaxPauliTermsPerSweep];
};
struct ExpectSweep : PauliSweep {
    uint32_t im_mask; // bit k: term k takes Im(conj(psi_j^x) psi_j) instead of Re
};
// Term k: c = cos(theta/2) and the real number v with w = -i sin(theta/2) i^ny = v (ny = popcount(x & z) odd, bit k of odd_mask)
// or i v (even); a sign per shard is folded into v.  full: a != b; otherwise a == b.
struct RotSweep : PauliSweep {
    double c[kMaxPauliTermsPerSweep], v[kMaxPauliTermsPerSweep];
    uint32_t odd_mask;
};

constexpr int kExpectGrid = 1024;     // workgroups of an expectation sweep at most = rows of partial sums (4 per CU)
constexpr size_t kExpectPartialDoubles = (size_t)kExpectGrid * kMaxPauliTermsPerSweep;
// The layout of a state's sweep scratch (qsim_state::d_expect; engine_state.h declares its allocator and accessors): the partial
// sums of the reducing sweep that runs, and behind them kResultRowBatch rows of kResultRowSlots results, one row per sweep, so that
// the results of up to kResultRowBatch sweeps travel in one copy behind one synchronisation.
constexpr int kResultRowBatch = 128, kResultRowSlots = kMaxPauliTermsPerSweep;
constexpr size_t kSweepResultDoubles = (size_t)kResultRowBatch * kResultRowSlots;
constexpr size_t kSweepScratchDoubles = kExpectPartialDoubles + kSweepResultDoubles;
int expect_slots(int count); // term slots of the instantiation a sweep of `count` terms runs in (1, 8, 16, 32)
// d_out[k] = sum_j s_k(j) |a_j|^2 (x == 0 and not full) or sum_j s_k(j) Re/Im(conj(b_(j^x)) a_j), for k < expect_slots(count);
// d_partial: kExpectPartialDoubles doubles of scratch.  a and b may be the same buffer.
hipError_t launch_expect(const LaunchCfg &cfg, const void *a, const void *b, bool f32, int n, const ExpectSweep &sw, double *d_partial,
                         double *d_out);
// out[k] = the sum of column k over `rows` rows of `kt` partial sums, added in a fixed order (the last step of every reducing sweep)
hipError_t launch_expect_final(hipStream_t stream, const double *d_partial, int rows, int kt, double *d_out);
// a_j' = c a_j + w (-1)^ny s(j) b_(j^x),  b_(j^x)' = c b_(j^x) + w s(j) a_j, term after term.
hipError_t launch_pauli_rot(const LaunchCfg &cfg, void *a, void *b, bool f32, int n, const RotSweep &sw);
// The same 2x2s, term after term, on the indices whose bits of `controls` are all 1 and nowhere else (crot.hip): one
// state, one buffer (sw.full is refused), controls != 0, inside the buffer and disjoint from sw.x.  A z bit on a control qubit is
// a constant sign there, folded into the term's v.
hipError_t launch_pauli_crot(const LaunchCfg &cfg, void *a, bool f32, int n, uint64_t controls, const RotSweep &sw);
// The backward sweep of an adjoint gradient over psi and lambda (two buffers, one state each: sw.full is refused).  From the LAST
// term of sw to the first: d_out[k] = sum over the pairs of s_k(j) Re (odd ny) or Im (even ny) of [conj(lambda_(j^x)) psi_j +
// (-1)^ny conj(lambda_j) psi_(j^x)]  (x == 0: sum_j s_k(j) Im conj(lambda_j) psi_j), then term k's 2x2 — c and v as for
// launch_pauli_rot, of MINUS theta_k — on psi and on lambda.  k < expect_slots(count); d_partial as for launch_expect.
hipError_t launch_pauli_adjoint(const LaunchCfg &cfg, void *psi, void *lam, bool f32, int n, const RotSweep &sw, double *d_partial, double *d_out);
// The same backward sweep on the indices whose bits of `controls` are all 1 and nowhere else (cadjoint.hip): the sums
// run over the pairs inside the control subspace, and psi and lambda are stepped back only there.  sw.full is refused, controls != 0,
// inside the buffer and disjoint from sw.x — and from every sw.z: a z bit on a control qubit would be a sign of the sum as well as of
// v, and no caller sends one, so it is refused, not folded.
hipError_t launch_pauli_cadjoint(const LaunchCfg &cfg, void *psi, void *lam, bool f32, int n, uint64_t controls, const RotSweep &sw, double *d_partial,
                                 double *d_out);
// Term k of a sum of strings with one x: c = coefficient times the non-zero component of i^ny times (-1)^ny; bit k of odd_mask: ny
// is odd, the term belongs to the imaginary part of the weight.
struct SumSweep : PauliSweep {
    double c[kMaxPauliTermsPerSweep];
    uint32_t odd_mask;
    bool accumulate; // dst += instead of dst =
};
// dst_i (=|+=) src_(i^x) (sum_even c_k s_k(i) + i sum_odd c_k s_k(i)), out of place: src and dst are different buffers.
hipError_t launch_pauli_sum(const LaunchCfg &cfg, const void *src, void *dst, bool f32, int n, const SumSweep &sw);
// dst_i <- d dst_i + a p_i + b q_i and d_out[0] = sum_i |dst_i|^2 of the values as stored (combine.hip).  d, a, b: (re, im),
// rounded once to the state's precision.  p != dst, q != dst; q == NULL: no third stream (b is not looked at); d == NULL or d == 0: dst
// is not loaded, whatever it holds.  A reducing sweep: d_partial as for launch_expect, cfg.grid_cap does not apply.
hipError_t launch_combine(const LaunchCfg &cfg, void *dst, const double *d, const void *p, const double *a, const void *q, const double *b, bool f32,
                          int n, double *d_partial, double *d_out);

// the partner index and every z must stay inside the buffer of 2^n amplitudes
inline bool check_sweep(const PauliSweep &sw, int n) {
    if (sw.count < 1 || sw.count > kMaxPauliTermsPerSweep || n < 0 || n > 40) return false;
    const uint64_t N = 1ULL << n;
    if (sw.x >= N) return false;
    for (int k = 0; k < sw.count; k++)
        if (sw.z[k] >= N) return false;
    return true;
}

// ---- geometry -----------------------------------------------------------------------------------------------------------------
constexpr int kTPB = 256;                     // 4 waves; a unit index's low 8 bits are the thread
constexpr int kTidBits = 8;
static_assert((1 << kTidBits) == kTPB, "unit index = (q << kTidBits) | tid");
// units per thread and trip: 8 independent 16-byte loads in flight (a paired sweep loads two units per unit visited)
constexpr int units_per_trip(bool paired) { return paired ? 4 : 8; }
// the adjoint sweep walks two buffers: the same 8 loads in flight are half as many units (a paired sweep keeps four units live per
// unit visited)
constexpr int adjoint_units_per_trip(bool paired) { return units_per_trip(paired) / 2; }

struct SweepGeom {      // by value: a kernel argument
    uint64_t units;     // 16-byte units to visit
    uint64_t low;       // unit-index bits below the inserted zero (all ones: nothing inserted)
    uint64_t x;         // partner amplitude = amplitude ^ x
    uint64_t amps;      // amplitudes in the buffer (guards the one-amplitude fp32 register)
    uint32_t odd_slot;  // fp32: the odd amplitude of a unit is visited too (0 only for x == 1 on one state: both members share the unit)
};

inline SweepGeom sweep_geom(uint64_t x, bool full, bool f32, int n) {
    const uint64_t N = 1ULL << n;
    const int as = f32 ? 1 : 0; // log2 amplitudes per unit
    SweepGeom g{};
    g.x = x;
    g.amps = N;
    g.odd_slot = 1;
    g.low = ~0ULL;
    uint64_t amps_visited = N;
    if (x != 0 && !full) { // one member of each pair: the index with the highest bit of x clear
        const int h = 63 - __builtin_clzll(x);
        amps_visited = N >> 1;
        if (h >= as) g.low = (1ULL << (h - as)) - 1ULL; // the zero is inserted at unit bit h - as
        else g.odd_slot = 0;                            // fp32, x == 1: every unit, one pair each
    }
    g.units = g.odd_slot ? (amps_visited >> as) : N >> as;
    if (g.units == 0) g.units = 1; // one fp32 amplitude
    return g;
}

// A sweep under controls (k_pauli_crot, k_pauli_cadjoint) visits the indices with every control bit 1 and, for x != 0, the highest bit h of x clear:
// 2^-c of what sweep_geom visits.  A unit index is expanded by inserting one fixed bit per set bit of `zeros` — the list of
// insertion positions in the unit index, as a bit set, taken lowest first (each insertion leaves the bits below its position and the
// bits inserted before it where they are).  Every inserted bit is a zero, so the expansion stays linear over OR, and the control
// bits are OR-ed in afterwards as the constant `ones`.  fp32: amplitude bit 0 is the slot inside a unit and is never inserted —
// x == 1 is odd_slot == 0 as in SweepGeom, and a control on qubit 0 leaves the odd slot of every visited unit as the only active
// one (first_slot == 1); the two cannot meet, controls and x are disjoint.
struct CtrlGeom {       // by value: a kernel argument
    uint64_t units;     // 16-byte units to visit
    uint64_t x;         // partner amplitude = amplitude ^ x
    uint64_t zeros;     // bit p: a zero is inserted at bit p of the unit index (h and the controls, but for amplitude bit 0 in fp32)
    uint64_t ones;      // the control bits of a unit's (even) amplitude index
    uint32_t odd_slot;  // as in SweepGeom
    uint32_t first_slot;// fp32: 1 when qubit 0 is a control (slot 0 is loaded and stored as it is)
};

inline CtrlGeom ctrl_geom(uint64_t controls, uint64_t x, bool f32, int n) {
    const uint64_t N = 1ULL << n;
    const int as = f32 ? 1 : 0;
    CtrlGeom g{};
    g.x = x;
    g.odd_slot = 1;
    uint64_t fixed = controls;
    if (x != 0) {
        const int h = 63 - __builtin_clzll(x);
        fixed |= 1ULL << h;
        if (h < as) g.odd_slot = 0;
    }
    g.first_slot = (uint32_t)(controls & (uint64_t)as);
    g.ones = controls & ~(uint64_t)as;
    g.zeros = (fixed & (N - 1ULL)) >> as;
    g.units = (N >> as) >> __builtin_popcountll(g.zeros);
    if (g.units == 0) g.units = 1; // one fp32 amplitude (no control fits such a register)
    return g;
}

// Workgroups of Kernel (kTPB threads, no dynamic LDS) resident at once, 0 when the query fails.  One figure per kernel and
// process: the devices of a cluster are of one kind.
template <auto Kernel>
int resident_grid() {
    static const int grid = [] {
        int dev = 0, per_cu = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, kTPB, 0) != hipSuccess || per_cu < 1)
            return 0;
        return per_cu * prop.multiProcessorCount;
    }();
    return grid;
}

// The grid of a sweep that REDUCES (k_expect, k_pauli_adjoint, k_pauli_cadjoint): the resident grid, at most kExpectGrid workgroups because the
// partial-sum buffer has that many rows, whatever LaunchCfg::grid_cap says — the sums are added row by row, so their bits depend on
// the grid, and equal calls must return equal bits whatever the option says.  (k_pauli_adjoint writes amplitudes too; each is
// written by one thread and would not care.)  The 32-slot instantiations of k_expect hold 3 workgroups per CU, the others 4 and more.
template <auto Kernel>
unsigned reducing_grid(uint64_t units, uint64_t per_block) {
    const int resident = resident_grid<Kernel>();
    const uint64_t cap = resident > 0 && resident < kExpectGrid ? resident : kExpectGrid;
    uint64_t grid = (units + per_block - 1) / per_block;
    if (grid > cap) grid = cap;
    return grid == 0 ? 1u : (unsigned)grid;
}
// The grid of a sweep that only WRITES, every output by one thread (k_pauli_rot, k_pauli_sum): QSIM_OPT_GRID_CAP > 0 caps it as it
// does for every kernel (a huge cap: one workgroup per block of units); otherwise the resident grid, and 1024 when the occupancy
// query fails.
template <auto Kernel>
unsigned writing_grid(const LaunchCfg &cfg, uint64_t units, uint64_t per_block) {
    const int resident = resident_grid<Kernel>();
    const uint64_t cap = cfg.grid_cap > 0 ? (uint64_t)cfg.grid_cap : resident > 0 ? (uint64_t)resident : 1024;
    uint64_t grid = (units + per_block - 1) / per_block;
    if (grid > cap) grid = cap;
    return grid == 0 ? 1u : (unsigned)grid;
}

// ---- which instantiation a launch runs in ---------------------------------------------------------------------------------------
// f(R{}, std::bool_constant<PAIRED>{}) for the state's precision and for whether the sweep has a partner
template <typename F>
hipError_t for_precision_and_pairing(bool f32, bool paired, F &&f) {
    if (f32) return paired ? f(float{}, std::true_type{}) : f(float{}, std::false_type{});
    return paired ? f(double{}, std::true_type{}) : f(double{}, std::false_type{});
}
// f(std::integral_constant<int, KT>{}) for KT = expect_slots(count)
template <typename F>
hipError_t for_term_slots(int count, F &&f) {
    switch (expect_slots(count)) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    default: return hipErrorInvalidValue;
    }
}

// ---- term records: what a kernel gets of a RotSweep or SumSweep, by value (scalar loads) -------------------------------------------
static_assert(kMaxPauliTermsPerSweep <= 32, "one bit per term in a record's `odd` and in a thread's parity mask");
// k_pauli_rot, k_pauli_crot (KT = kMaxPauliTermsPerSweep, terms of +theta) and k_pauli_adjoint, k_pauli_cadjoint (KT =
// expect_slots(count), terms of -theta)
template <typename R, int KT>
struct RotTerms {
    uint64_t z[KT];     // unused slots: 0
    R c[KT], v[KT];     // rounded once to the state's precision by the host
    uint32_t odd;       // bit k: ny is odd — w = v is real and a's sign is opposite to b's (the adjoint sweep sums the real part of its
                        // bracket); else w = i v (the imaginary part)
    int32_t count;
};
static_assert(sizeof(RotTerms<double, kMaxPauliTermsPerSweep>) <= 1024, "term records stay well inside the 4 KiB of kernel arguments");
// z, c, odd and count of the sweep's terms, and v where the record has one (RotTerms; adjoint.hip's SumTerms has none)
template <typename Rec, typename Sweep>
void fill_terms(Rec &rec, const Sweep &sw) {
    using R = std::remove_reference_t<decltype(rec.c[0])>;
    constexpr int slots = (int)(sizeof(rec.z) / sizeof(rec.z[0]));
    for (int k = 0; k < sw.count && k < slots; k++) {
        rec.z[k] = sw.z[k];
        rec.c[k] = (R)sw.c[k];
        if constexpr (std::is_same_v<Sweep, RotSweep>) rec.v[k] = (R)sw.v[k];
    }
    rec.odd = sw.odd_mask;
    rec.count = sw.count;
}

// ---- device helpers -----------------------------------------------------------------------------------------------------------
template <typename R> struct Vec16;
template <> struct Vec16<double> { using type = double2; };
template <> struct Vec16<float> { using type = float4; };

__device__ __forceinline__ double flip(double v, uint32_t sign_bit31) {
    return __hiloint2double(__double2hiint(v) ^ (int)sign_bit31, __double2loint(v));
}
__device__ __forceinline__ float flip(float v, uint32_t sign_bit31) { return __uint_as_float(__float_as_uint(v) ^ sign_bit31); }

// unit index -> its (even) amplitude index
template <typename R>
__device__ __forceinline__ uint64_t expand(const SweepGeom &g, uint64_t t) {
    return (((t & ~g.low) << 1) | (t & g.low)) << (sizeof(R) == 8 ? 0 : 1);
}
// the same under controls (k_pauli_crot, k_pauli_cadjoint): unit-index bits -> their places in the (even) amplitude index, the fixed
// bits left zero
template <typename R>
__device__ __forceinline__ uint64_t spread(const CtrlGeom &g, uint64_t t) {
    for (uint64_t f = g.zeros; f != 0; f &= f - 1ULL) { // uniform: the positions come off a scalar register, lowest first
        const uint64_t low = (f & (0ULL - f)) - 1ULL;
        t = ((t & ~low) << 1) | (t & low);
    }
    return t << (sizeof(R) == 8 ? 0 : 1);
}
// the unit that holds amplitude `amp` (even for fp32)
template <typename R>
__device__ __forceinline__ typename Vec16<R>::type load_unit(const R *p, uint64_t amp) {
    return *reinterpret_cast<const typename Vec16<R>::type *>(p + 2 * amp);
}
// the same for a register that may be a single fp32 amplitude: 8 bytes long, no unit
template <typename R>
__device__ __forceinline__ typename Vec16<R>::type load_unit_or_one(const SweepGeom &g, const R *p, uint64_t amp) {
    if constexpr (sizeof(R) == 4) if (g.amps < 2) {
        const float2 one = *reinterpret_cast<const float2 *>(p);
        float4 v{};
        v.x = one.x;
        v.y = one.y;
        return v;
    }
    return load_unit(p, amp);
}
// (-1)^popcount(j & z) as a sign bit (bit 31) for flip — j: the index bits that are uniform over the workgroup (scalar), or a thread's
// own — and the same for the odd fp32 slot of a unit, whose index has bit 0 set
__device__ __forceinline__ uint32_t parity_sign(uint64_t j, uint64_t z) { return ((uint32_t)__builtin_popcountll(j & z) & 1u) << 31; }
__device__ __forceinline__ uint32_t odd_slot_sign(uint32_t sg, uint64_t z) { return sg ^ ((uint32_t)(z & 1ULL) << 31); }
// One state's visited unit and its partner's unit as they are stored, from (xr, xi) of the visited member's slots and (yr, yi) of
// the partner's.  fp32: selects on values, so that every store stays one 16-byte store; `same`: x == 1 on one state, the pair is
// the unit; `swapped`: x is odd, the partner sits in the other half of its unit.
template <typename R, int A>
__device__ __forceinline__ typename Vec16<R>::type own_unit(bool same, const R (&xr)[A], const R (&xi)[A], const R (&yr)[A], const R (&yi)[A]) {
    using V = typename Vec16<R>::type;
    if constexpr (A == 1) return V{xr[0], xi[0]};
    else return V{xr[0], xi[0], same ? yr[0] : xr[1], same ? yi[0] : xi[1]};
}
template <typename R, int A>
__device__ __forceinline__ typename Vec16<R>::type partner_unit(bool swapped, const R (&yr)[A], const R (&yi)[A]) {
    using V = typename Vec16<R>::type;
    if constexpr (A == 1) return V{yr[0], yi[0]};
    else return V{swapped ? yr[1] : yr[0], swapped ? yi[1] : yi[0], swapped ? yr[0] : yr[1], swapped ? yi[0] : yi[1]};
}

// The 2x2 of one rotation term on one pair, sv = s(j) v (evolve.hip has the rule): shared by k_pauli_rot and k_pauli_adjoint.
template <typename R>
__device__ __forceinline__ void rotate_pair(R &ar, R &ai, R &br, R &bi, R c, R sv, bool odd) {
    const R pr = odd ? br : bi, pi = odd ? bi : br;   // w b = sv (br, bi) or sv (-bi, br); a's sign: -1 for odd ny
    const R qr = odd ? ar : ai, qi = odd ? ai : ar;   // w a likewise
    const R nar = fma(-sv, pr, c * ar), nai = fma(odd ? -sv : sv, pi, c * ai);
    const R nbr = fma(odd ? sv : -sv, qr, c * br), nbi = fma(sv, qi, c * bi);
    ar = nar, ai = nai, br = nbr, bi = nbi;
}
// x == 0: a' = (c + i sv) a
template <typename R>
__device__ __forceinline__ void rotate_diag(R &ar, R &ai, R c, R sv) {
    const R nr = fma(-sv, ai, c * ar), ni = fma(sv, ar, c * ai);
    ar = nr, ai = ni;
}

} // namespace qsim
#endif
