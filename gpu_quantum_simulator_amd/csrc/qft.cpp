// qft.cpp — the quantum Fourier transform on any k qubits of the register: the plan (the one place that sizes the digits and says
// which pass writes which buffer), the record a pass hands its kernel, and the entry points.  The kernel is qft.hip's;
// qft.h has the pass rule they share.  The call settles the state, launches one sweep per digit on the state's stream and returns
// without waiting.  A pass that moves bits reads one buffer and writes the other; the second buffer is second_buffer()'s (pauli.cpp:
// the idle spare buffer, else d_adjoint), and the passes that write out of place are even in number, so the state ends where it began.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "engine_state.h"
#include "matrix.h" // kMatrixCoefDoubles: the size of a staging slot
#include "qft.h"

using namespace qsim;

static_assert(kQftMaxDigitBits + 2 <= qft_tile_bits(false), "a ten-bit digit on high qubits leaves the tile two padding bits");
static_assert(sizeof(QftPassRec) <= kMatrixCoefDoubles * sizeof(double), "a record fits a staging slot");
static_assert(qft_tile_bits(true) <= kQftMaxTileBits && qft_tile_bits(false) <= kQftMaxTileBits, "the record's per-bit tables hold a tile");

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
// The digit cap the plan chooses for itself (DESIGN §7o has the figures).  Up to ten qubits: one digit, one sweep in place, whatever the
// runs — a second sweep costs more than the 64-byte runs of a ten-bit digit on high qubits do.  More than ten: digits of at most
// nine bits, which leave the fp64 tile three padding bits.  That is a sweep more than ten-bit digits need at k = 19, 20 and 28 to 30, and
// it is still the faster split there: at n = 30 a ten-bit digit on high qubits costs 2.3 sweeps of the same bytes, a seven- or
// eight-bit one 1.0 to 1.3.
static constexpr int kQftLongDigitBits = 9;
static int own_cap(int k) { return k <= kQftMaxDigitBits ? kQftMaxDigitBits : kQftLongDigitBits; }

bool qsim::qft_plan(const int *qubits, int k, int n, bool f32, int max_digit_bits, QftPlan *out) {
    uint64_t reg;
    if (n < 0 || n > 40 || k < 0 || k > n || max_digit_bits < 0 || max_digit_bits > kQftMaxDigitBits) return false;
    if (!qubit_list_mask(qubits, k, n, 0, &reg)) return false;
    QftPlan pl{};
    pl.n = n, pl.k = k, pl.f32 = f32;
    std::copy(qubits, qubits + k, pl.qubits);
    const int cap = max_digit_bits ? max_digit_bits : own_cap(k);
    const int tile_bits = std::min(qft_tile_bits(f32), n);
    pl.passes = (k + cap - 1) / cap;
    pl.tiles = 1ULL << (n - tile_bits);
    pl.units = (1ULL << n) >> (f32 ? 1 : 0);
    if (pl.units == 0) pl.units = 1; // one fp32 amplitude
    pl.trips_at_cap = trips_at_cap(pl.tiles, 1, kQftGridCap);
    // the digits as even as the cap allows: the same sweeps, and every bit a digit is short of the cap is a padding bit more
    const int moving = pl.passes - 1;
    for (int p = 0, first = 0; p < pl.passes; p++) {
        QftPass &ps = pl.pass[p];
        const int left = pl.passes - p;
        ps.first = first, ps.kp = k - first, ps.d = (ps.kp + left - 1) / left, ps.tile_bits = tile_bits;
        ps.oop = p < moving || (moving & 1); // an odd number of moving passes: the last one goes back to the first buffer
        const int nr = ps.kp - ps.d, *Q = pl.qubits + first;
        uint64_t digit = 0;
        for (int m = 0; m < ps.d; m++) digit |= 1ULL << Q[nr + m];
        ps.in_mask = pad_subset(digit, 0, tile_bits, n);
        // where the tile's bits are afterwards: bit i of r moves from Q[i] to Q[d + i], u lands on Q[0 .. d), the rest stays
        uint64_t sub = 0;
        for (int i = 0; i < ps.kp; i++) sub |= 1ULL << Q[i];
        ps.out_mask = ps.in_mask & ~sub;
        for (int m = 0; m < ps.d; m++) ps.out_mask |= 1ULL << Q[m];
        for (int i = 0; i < nr; i++)
            if ((ps.in_mask >> Q[i]) & 1ULL) ps.out_mask |= 1ULL << Q[ps.d + i];
        first += ps.d;
    }
    *out = pl;
    return true;
}

QftPassRec qsim::qft_pass_record(const QftPlan &pl, int p, bool inverse) {
    const QftPass &ps = pl.pass[p];
    const int d = ps.d, nr = ps.kp - d, G = qft_round_bits(pl.f32), full_bits = qft_tile_bits(pl.f32), *Q = pl.qubits + ps.first;
    QftPassRec rec{};
    rec.d = d, rec.kp = ps.kp, rec.nr = nr, rec.elems = 1u << ps.tile_bits, rec.inverse = inverse ? 1u : 0u;
    rec.scale = std::ldexp(d & 1 ? M_SQRT1_2 : 1.0, -(d / 2));
    int where_in_sub[64], slot_of[64]; // per qubit: its place in the sub-register (-1: outside), the slot bit of a padding qubit
    std::fill(where_in_sub, where_in_sub + 64, -1);
    for (int i = 0; i < ps.kp; i++) where_in_sub[Q[i]] = i, rec.sub_mask |= 1ULL << Q[i];
    for (int i = 0; i < nr; i++) rec.r_from[i] = (uint8_t)Q[i], rec.r_to[i] = (uint8_t)Q[d + i];
    // in: a digit qubit Q[nr + m] goes to slot bit m, the padding qubits above the digit in ascending order, then the bits a small
    // register does not have
    int i = 0, pads = 0;
    for (int q = 0; q < pl.n; q++) {
        if (!((ps.in_mask >> q) & 1ULL)) continue;
        const int at = where_in_sub[q];
        slot_of[q] = at >= nr ? at - nr : d + pads++;
        rec.in_addr[i] = 1ULL << q;
        rec.in_lds[i++] = (uint16_t)qft_swizzle(1u << slot_of[q], G);
    }
    const int first_absent = d + pads;
    for (int b = first_absent; i < full_bits; i++, b++) rec.in_lds[i] = (uint16_t)qft_swizzle(1u << b, G);
    // out, in the order of the output addresses: Q[m] holds bit m of u, read from the bit-reversed slot; Q[d + j] holds bit j of r,
    // which came in on the padding qubit Q[j]; an environment qubit is where it was
    i = 0;
    for (int q = 0; q < pl.n; q++) {
        if (!((ps.out_mask >> q) & 1ULL)) continue;
        const int at = where_in_sub[q];
        rec.out_addr[i] = 1ULL << q;
        if (at >= 0 && at < d) {
            rec.out_u[i] = (uint16_t)(1u << at);
            rec.out_lds[i] = (uint16_t)qft_swizzle(1u << (d - 1 - at), G);
        } else if (at >= d) {
            rec.out_r[i] = 1ULL << (at - d);
            rec.out_lds[i] = (uint16_t)qft_swizzle(1u << slot_of[Q[at - d]], G);
        } else {
            rec.out_lds[i] = (uint16_t)qft_swizzle(1u << slot_of[q], G);
        }
        i++;
    }
    for (int b = first_absent; i < full_bits; i++, b++) rec.out_lds[i] = (uint16_t)qft_swizzle(1u << b, G);
    return rec;
}

static int to_plan(const char *who, const int *qubits, int k, int n, bool f32, int max_digit_bits, QftPlan *p) {
    if (!qft_plan(qubits, k, n, f32, max_digit_bits, p))
        return fail(QSIM_ERR_ARG, "%s: 0 to %d distinct qubits inside the register of %d and a digit cap of 0 (the plan's own) to %d bits", who, n, n,
                    kQftMaxDigitBits);
    return QSIM_OK;
}

extern "C" int qsim_apply_qft_max_digit_bits(void) { return kQftMaxDigitBits; }

extern "C" int qsim_apply_qft_plan(const int *qubits, int k, int num_q, int precision_bits, int max_digit_bits, int *passes, int *digit_bits,
                                   int *out_of_place, uint64_t *tile_mask, uint64_t *tiles, uint64_t *units, long *trips_per_workgroup) {
    const char *who = "qsim_apply_qft_plan";
    if (!passes || !digit_bits || !out_of_place || !tile_mask || !tiles || !units || !trips_per_workgroup) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    QftPlan p;
    QSIM_TRY(to_plan(who, qubits, k, num_q, precision_bits == 32, max_digit_bits, &p));
    *passes = p.passes, *tiles = p.tiles, *units = p.units, *trips_per_workgroup = p.trips_at_cap;
    for (int i = 0; i < p.passes; i++) digit_bits[i] = p.pass[i].d, out_of_place[i] = p.pass[i].oop ? 1 : 0, tile_mask[i] = p.pass[i].in_mask;
    return QSIM_OK;
}

// ---- the call ---------------------------------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_qft_sweeps{0};
extern "C" uint64_t qsim_qft_sweeps_launched(void) { return g_qft_sweeps.load(); }

extern "C" int qsim_apply_qft(qsim_state *s, const int *qubits, int k, int inverse, int max_digit_bits) {
    const char *who = "qsim_apply_qft";
    if (!s) return fail(QSIM_ERR_ARG, "%s: NULL state", who);
    QftPlan p;
    QSIM_TRY(to_plan(who, qubits, k, s->n, s->f32, max_digit_bits, &p));
    if (qsim_holds_nothing(s) || p.passes == 0) return QSIM_OK; // the zero vector stays the zero vector; no qubit: the identity
    QSIM_TRY(await_buffer(s));
    QSIM_TRY(settle(s));
    // everything that can fail for want of memory comes before the state is touched
    void *other = nullptr;
    if (p.pass[0].oop) QSIM_TRY(second_buffer(s, &other));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    void *at = s->amps;
    for (int i = 0; i < p.passes; i++) {
        void *to = p.pass[i].oop ? (at == s->amps ? other : s->amps) : at;
        const QftPassRec rec = qft_pass_record(p, i, inverse != 0);
        QSIM_TRY(stage_sweep_operand(s, &rec, sizeof rec)); // ordered on the stream behind the pass before, which read the same scratch
        QSIM_TRY(launched("qsim_apply_qft:", launch_qft_pass(cfg, at, to, p, i, rec, reinterpret_cast<const QftPassRec *>(sweep_coef_staging(s)))));
        g_qft_sweeps++;
        at = to;
    }
    if (at != s->amps) return fail(QSIM_ERR_DEVICE, "%s: the passes left the state in its second buffer", who); // the plan's parity rule forbids it
    return QSIM_OK;
}
