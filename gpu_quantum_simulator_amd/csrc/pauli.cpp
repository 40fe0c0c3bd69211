// pauli.cpp — the host side of Pauli strings: expectation values <psi|P|psi> (expect.hip; DESIGN "Expectation values"),
// rotations exp(-i theta/2 P) applied in the caller's order (evolve.hip; DESIGN "Pauli rotations"), the same under control qubits
// (crot.hip; DESIGN "Controlled Pauli rotations") and adjoint-mode gradients of
// <H> with respect to the angles (adjoint.hip, cadjoint.hip through controlled rotations and diagonal.hip through the phases exp(-i gamma D)
// of a table; DESIGN "Adjoint gradients", §7k).  pauli_sweep.h has what the sweeps share.  Every
// entry point opens with settle() and then only touches qsim_state's buffer, stream and d_expect; expectation values read the
// buffer, rotations write it, a gradient call writes it and a second buffer of the same size (the spare one, or d_adjoint) and
// leaves the state as it found it.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>

#include "diagonal.h" // a gradient's diagonal steps and the diagonal part of its observable
#include "engine_state.h"
#include "matrix.h" // kMatrixCoefDoubles: sweep_coef_staging
#include "pauli_sweep.h"
#include "subset_sweep.h" // trips_at_cap

using namespace qsim;

// ---- what both kinds share ----------------------------------------------------------------------------------------------------
// i^k is real (k even) or imaginary (k odd); its non-zero component: 1, 1, -1, -1 for k = 0, 1, 2, 3 mod 4
static double pauli_phase(int k) { return (k & 2) ? -1.0 : 1.0; }
// <P> = i^ny (c + (-1)^ny conj c) summed over the pairs = 2 i^ny Re c (ny even) or 2 i^(ny+1) Im c (odd): 2 Re c, -2 Im c, -2 Re c,
// 2 Im c for ny = 0, 1, 2, 3 mod 4; x == 0: the plain signed norm
static double expect_factor(uint64_t x, int ny) { return x == 0 ? 1.0 : 2.0 * pauli_phase(ny + (ny & 1)); }
// w = -i sin(theta/2) i^ny = i^(ny+3) sin(theta/2): -i sn, sn, i sn, -sn for ny = 0, 1, 2, 3 mod 4; v is its non-zero component
static double rotation_v(int ny, double sn) { return pauli_phase(ny + 3) * sn; }
// Z on rank qubits (mask bits from m up): a sign per shard
static double rank_sign(uint64_t rank, uint64_t z, int m) { return (__builtin_popcountll(rank & (z >> m)) & 1) ? -1.0 : 1.0; }

// qsim_internal.h says what is checked; the single-state entry points call it through check_terms, the cluster's through physical_terms
int qsim::check_pauli_terms(int (*report)(int, const char *, ...), const char *who, int n, const uint64_t *x_masks, const uint64_t *z_masks,
                            const void *third, const double *numbers, long num_terms, const char *number, long first) {
    if (num_terms < 0) return report(QSIM_ERR_ARG, "%s: negative term count", who);
    if (num_terms > 0 && (!x_masks || !z_masks || !third)) return report(QSIM_ERR_ARG, "%s: NULL argument", who);
    const uint64_t nmask = index_mask(n);
    for (long t = 0; t < num_terms; t++) {
        if ((x_masks[t] | z_masks[t]) & ~nmask) return report(QSIM_ERR_ARG, "%s: term %ld names a qubit outside the %d-qubit register", who, first + t, n);
        if (numbers && !std::isfinite(numbers[t])) return report(QSIM_ERR_ARG, "%s: term %ld has a non-finite %s", who, first + t, number);
    }
    return QSIM_OK;
}
static int check_terms(const char *who, const qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, const void *third, const double *numbers,
                       long num_terms, const char *number = "angle") {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    return check_pauli_terms(fail, who, s->n, x_masks, z_masks, third, numbers, num_terms, number);
}

// ---- the sweep scratch and its result rows ------------------------------------------------------------------------------------------
// s->d_expect has ONE owner, here: every file that needs a part of it calls alloc_sweep_scratch and then an accessor
// (engine_state.h), and pauli_sweep.h has the sizes.
int qsim::alloc_sweep_scratch(qsim_state *s) {
    if (!s->d_expect) HIP_TRY(hipMalloc((void **)&s->d_expect, kSweepScratchDoubles * sizeof(double)));
    return QSIM_OK;
}
double *qsim::sweep_partials(qsim_state *s) { return s->d_expect; }
double *qsim::sweep_result_row(qsim_state *s) { return s->d_expect + kExpectPartialDoubles; }
// The operand of qsim_apply_matrix ALIASES the partial sums, on purpose: everything that touches either is ordered on the state's
// stream, and no reducing sweep is in flight while a matrix sweep reads its coefficients.
static_assert(kMatrixCoefDoubles <= kExpectPartialDoubles, "the largest matrix operand fits in the partial-sum region");
double *qsim::sweep_coef_staging(qsim_state *s) { return sweep_partials(s); }

// ---- a second buffer of the state's size, outside a flush --------------------------------------------------------------------------
// lambda of a gradient call, the other side of a Fourier transform's moving passes: the spare buffer, which is idle outside a flush,
// else d_adjoint, allocated on first use and the state's own from then on.  Call it before the state is touched.
int qsim::second_buffer(qsim_state *s, void **out) {
    void *buf = s->spare && s->spare != s->amps ? s->spare : s->d_adjoint;
    if (!buf) {
        HIP_TRY(hipMalloc(&buf, s->amp_bytes() << s->n));
        s->d_adjoint = buf;
    }
    *out = buf;
    return QSIM_OK;
}

int qsim::fetch_sweep_results(qsim_state *s, int count, double *out) {
    HIP_TRY(hipMemcpyAsync(out, sweep_result_row(s), (size_t)count * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return QSIM_OK;
}
// launch(r, d_row) queues the sweep of row r < rows on the state's stream; scatter(r, row) gets its kResultRowSlots sums on the
// host.  Batch after batch in order of r; what a row means is the caller's.
template <typename Launch, typename Scatter>
static int sweep_result_rows(qsim_state *s, size_t rows, Launch launch, Scatter scatter) {
    double *d_rows = sweep_result_row(s);
    std::vector<double> host(kSweepResultDoubles);
    for (size_t first = 0; first < rows; first += kResultRowBatch) {
        const size_t last = std::min(rows, first + (size_t)kResultRowBatch);
        for (size_t r = first; r < last; r++) QSIM_TRY(launch(r, d_rows + (r - first) * kResultRowSlots));
        HIP_TRY(hipMemcpyAsync(host.data(), d_rows, (last - first) * kResultRowSlots * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        for (size_t r = first; r < last; r++) scatter(r, host.data() + (r - first) * kResultRowSlots);
    }
    return QSIM_OK;
}

// ---- expectation values ---------------------------------------------------------------------------------------------------------
// Terms per sweep: kPauliTermsPerSweep by measurement (DESIGN); QSIM_PAULI_TERMS_PER_SWEEP = 8 | 16 | 32 in the environment
// overrides it for tools/expect_bench.py, which times the candidates against each other.
static constexpr int kPauliTermsPerSweep = 32;
static int pauli_terms_per_sweep() {
    static const int k = [] {
        const char *e = getenv("QSIM_PAULI_TERMS_PER_SWEEP");
        const int v = e ? atoi(e) : 0;
        return v == 8 || v == 16 || v == 32 ? v : kPauliTermsPerSweep;
    }();
    return k;
}
extern "C" int qsim_pauli_terms_per_sweep(void) { return pauli_terms_per_sweep(); }

// The sweeps of a term list: terms in order of x (equal x: caller's order), every run of equal x cut into pieces of K.
struct PauliSweeps {
    std::vector<long> order;                     // term indices, grouped
    std::vector<std::pair<long, int>> sweeps;    // (first position in `order`, terms)
};
static PauliSweeps pauli_sweeps(const uint64_t *x, uint64_t x_keep, long num) {
    PauliSweeps p;
    p.order.resize((size_t)num);
    for (long t = 0; t < num; t++) p.order[(size_t)t] = t;
    std::stable_sort(p.order.begin(), p.order.end(), [&](long a, long b) { return (x[a] & x_keep) < (x[b] & x_keep); });
    const int K = pauli_terms_per_sweep();
    for (long i = 0; i < num;) {
        long e = i + 1;
        while (e < num && (x[p.order[(size_t)e]] & x_keep) == (x[p.order[(size_t)i]] & x_keep)) e++;
        for (; i < e; i += K) p.sweeps.emplace_back(i, (int)std::min<long>(K, e - i));
        i = e;
    }
    return p;
}

extern "C" int qsim_pauli_sweeps(const uint64_t *x_masks, long num_terms, long *sweeps) {
    if (!sweeps || num_terms < 0 || (num_terms > 0 && !x_masks)) return fail(QSIM_ERR_ARG, "qsim_pauli_sweeps: bad argument");
    *sweeps = (long)pauli_sweeps(x_masks, ~0ULL, num_terms).sweeps.size();
    return QSIM_OK;
}

int qsim::expect_paulis_shard(qsim_state *s, const void *partner, uint64_t rank, const uint64_t *X, const uint64_t *Z, long num, double *out) {
    if (!s || num < 0 || (num > 0 && (!X || !Z || !out))) return fail(QSIM_ERR_ARG, "expectation: NULL argument or negative term count");
    if (num == 0) return QSIM_OK;
    const int m = s->n;
    const uint64_t mmask = index_mask(m), x_rank = X[0] >> m;
    for (long t = 0; t < num; t++)
        if ((X[t] >> m) != x_rank) return fail(QSIM_ERR_ARG, "expectation: terms of one shard call must pair the same shards");
    if ((x_rank != 0) != (partner != nullptr)) return fail(QSIM_ERR_ARG, "expectation: a partner buffer goes with x on rank qubits, and only with it");
    QSIM_TRY(settle(s));
    QSIM_TRY(alloc_sweep_scratch(s));
    const PauliSweeps plan = pauli_sweeps(X, mmask, num);
    const LaunchCfg cfg{s->stream, s->grid_cap};
    return sweep_result_rows(
        s, plan.sweeps.size(),
        [&](size_t w, double *d_row) {
            ExpectSweep sw{};
            sw.x = X[plan.order[(size_t)plan.sweeps[w].first]] & mmask;
            sw.full = x_rank != 0;
            sw.count = plan.sweeps[w].second;
            for (int k = 0; k < sw.count; k++) {
                const long t = plan.order[(size_t)(plan.sweeps[w].first + k)];
                sw.z[k] = Z[t] & mmask;
                if (__builtin_popcountll(X[t] & Z[t]) & 1) sw.im_mask |= 1u << k;
            }
            return launched("expectation sweep", launch_expect(cfg, s->amps, partner ? partner : s->amps, s->f32, m, sw, sweep_partials(s), d_row));
        },
        [&](size_t w, const double *row) {
            for (int k = 0; k < plan.sweeps[w].second; k++) {
                const long t = plan.order[(size_t)(plan.sweeps[w].first + k)];
                out[t] = expect_factor(X[t], __builtin_popcountll(X[t] & Z[t])) * rank_sign(rank, Z[t], m) * row[k];
            }
        });
}

extern "C" int qsim_expect_paulis(qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, double *out) {
    QSIM_TRY(check_terms("qsim_expect_paulis", s, x_masks, z_masks, out, nullptr, num_terms));
    return expect_paulis_shard(s, nullptr, 0, x_masks, z_masks, num_terms, out);
}

// ---- rotations ------------------------------------------------------------------------------------------------------------------
// A term that is X or Y on a single qubit is a 2x2 for the gate queue; every other term goes to an in-place sweep, and consecutive
// sweep terms with one x mask (and one control mask, where there are controls: below) share a sweep.
// Terms per sweep: 32, the record count of k_pauli_rot; not backed by a measurement yet (DESIGN "Pauli rotations").
static constexpr int kPauliRotationsPerSweep = kMaxPauliTermsPerSweep;
extern "C" int qsim_pauli_rotations_per_sweep(void) { return kPauliRotationsPerSweep; }

static std::atomic<uint64_t> g_sweeps_launched{0};
extern "C" uint64_t qsim_pauli_rotation_sweeps_launched(void) { return g_sweeps_launched.load(); }

long qsim::rotation_sweeps(long run_length) { return (run_length + kPauliRotationsPerSweep - 1) / kPauliRotationsPerSweep; }

// with at most one control: the 2x2, or its 4x4 under the control
static bool is_gate(uint64_t c, uint64_t x, uint64_t z, uint64_t local_mask) {
    return __builtin_popcountll(c) <= 1 && __builtin_popcountll(x) == 1 && (z & ~x) == 0 && (x & local_mask) != 0;
}

std::vector<RotRoute> qsim::route_rotations(const uint64_t *X, const uint64_t *Z, long num, uint64_t local_mask, const uint64_t *C) {
    std::vector<RotRoute> out;
    auto c = [&](long t) { return C ? C[t] : 0; };
    for (long t = 0; t < num;) {
        if (is_gate(c(t), X[t], Z[t], local_mask)) {
            out.push_back({t, 1, true});
            t++;
            continue;
        }
        long e = t + 1;
        while (e < num && X[e] == X[t] && c(e) == c(t) && !is_gate(c(e), X[e], Z[e], local_mask)) e++;
        out.push_back({t, e - t, false});
        t = e;
    }
    return out;
}

void qsim::pauli_rot_1q(bool y, double theta, double *U) {
    const double c = std::cos(0.5 * theta), sn = std::sin(0.5 * theta);
    const double ux[8] = {c, 0, 0, -sn, 0, -sn, c, 0}, uy[8] = {c, 0, -sn, 0, sn, 0, c, 0};
    std::copy(y ? uy : ux, (y ? uy : ux) + 8, U);
}

// `count` terms of one x as one sweep of the angles sign * theta (-1: the inverse, for the way back of a gradient) on the shard
// `rank` of local mask `mmask` (m bits); x carries the rank bits too, ny counts them, the sweep's masks are the local part.
static RotSweep rot_sweep(uint64_t x, const uint64_t *Z, const double *thetas, int count, double sign, uint64_t rank, uint64_t mmask, int m) {
    RotSweep sw{};
    sw.x = x & mmask;
    sw.full = (x & ~mmask) != 0;
    sw.count = count;
    for (int k = 0; k < count; k++) {
        const double half = sign * 0.5 * thetas[k];
        const int ny = __builtin_popcountll(x & Z[k]);
        sw.z[k] = Z[k] & mmask;
        sw.c[k] = std::cos(half);
        sw.v[k] = rotation_v(ny, std::sin(half)) * rank_sign(rank, Z[k], m);
        if (ny & 1) sw.odd_mask |= 1u << k;
    }
    return sw;
}

int qsim::pauli_rot_run(qsim_state *s, void *partner, uint64_t rank, uint64_t x, const uint64_t *Z, const double *thetas, long count) {
    if (!s || count < 0 || (count > 0 && (!Z || !thetas))) return fail(QSIM_ERR_ARG, "rotation: NULL argument or negative term count");
    const int m = s->n;
    const uint64_t mmask = index_mask(m);
    if (((x >> m) != 0) != (partner != nullptr)) return fail(QSIM_ERR_ARG, "rotation: a partner buffer goes with x on rank qubits, and only with it");
    if (count == 0 || (!partner && qsim_holds_nothing(s))) return QSIM_OK; // rotations map the zero vector to itself
    QSIM_TRY(settle(s));
    HIP_TRY(hipSetDevice(s->device)); // a cluster drives several devices from one thread, and settle() may have had nothing to do
    const LaunchCfg cfg{s->stream, s->grid_cap};
    for (long first = 0; first < count; first += kPauliRotationsPerSweep) {
        const RotSweep sw = rot_sweep(x, Z + first, thetas + first, (int)std::min<long>(kPauliRotationsPerSweep, count - first), 1.0, rank, mmask, m);
        QSIM_TRY(launched("rotation sweep", launch_pauli_rot(cfg, s->amps, partner ? partner : s->amps, s->f32, m, sw)));
        g_sweeps_launched++;
    }
    return QSIM_OK;
}

extern "C" int qsim_pauli_rotation_plan(const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, long *sweeps, long *queued_as_gates) {
    if (num_terms < 0) return fail(QSIM_ERR_ARG, "qsim_pauli_rotation_plan: negative term count");
    if (!sweeps || !queued_as_gates || (num_terms > 0 && (!x_masks || !z_masks))) return fail(QSIM_ERR_ARG, "qsim_pauli_rotation_plan: NULL argument");
    *sweeps = *queued_as_gates = 0;
    for (const RotRoute &r : route_rotations(x_masks, z_masks, num_terms, ~0ULL)) {
        if (r.gate) ++*queued_as_gates;
        else *sweeps += rotation_sweeps(r.count);
    }
    return QSIM_OK;
}

// ---- controlled rotations (crot.hip; DESIGN "Controlled Pauli rotations") ---------------------------------------------------------
// Term t acts as exp(-i theta/2 P_t) where every qubit of c_masks[t] is 1 and as the identity elsewhere.  route_rotations has the
// rule: one control on a single X or Y is a 4x4 for the gate queue, every other controlled term goes to a sweep of the control
// subspace, and a run shares sweeps only under one control mask.  A term without controls takes the uncontrolled path.
static int check_controls(const char *who, int n, const uint64_t *C, const uint64_t *X, const uint64_t *Z, long num, long first = 0) {
    for (long t = 0; C && t < num; t++) { // first: as for check_pauli_terms
        if (C[t] & ~index_mask(n)) return fail(QSIM_ERR_ARG, "%s: term %ld names a control qubit outside the %d-qubit register", who, first + t, n);
        if (C[t] & (X[t] | Z[t])) return fail(QSIM_ERR_ARG, "%s: term %ld: a control qubit carries a Pauli factor", who, first + t);
    }
    return QSIM_OK;
}

// [[I, 0], [0, R]] on (control, target) as qsim_apply_2q takes it: row / column index = (bit q_hi, bit q_lo), R = pauli_rot_1q
static void controlled_rot_2q(bool y, double theta, bool control_is_hi, double *U) {
    double R[8];
    pauli_rot_1q(y, theta, R);
    std::fill(U, U + 32, 0.0);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            const int rc = control_is_hi ? r >> 1 : r & 1, cc = control_is_hi ? c >> 1 : c & 1;
            const int rt = control_is_hi ? r & 1 : r >> 1, ct = control_is_hi ? c & 1 : c >> 1;
            if (rc != cc) continue;
            if (rc) U[2 * (4 * r + c)] = R[2 * (2 * rt + ct)], U[2 * (4 * r + c) + 1] = R[2 * (2 * rt + ct) + 1];
            else U[2 * (4 * r + c)] = rt == ct ? 1.0 : 0.0;
        }
}

// One run under the control mask c != 0, on a single state
static int controlled_rot_run(qsim_state *s, uint64_t c, uint64_t x, const uint64_t *Z, const double *thetas, long count) {
    if (count == 0 || qsim_holds_nothing(s)) return QSIM_OK;
    QSIM_TRY(settle(s));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    for (long first = 0; first < count; first += kPauliRotationsPerSweep) {
        const RotSweep sw = rot_sweep(x, Z + first, thetas + first, (int)std::min<long>(kPauliRotationsPerSweep, count - first), 1.0, 0, index_mask(s->n), s->n);
        QSIM_TRY(launched("controlled rotation sweep", launch_pauli_crot(cfg, s->amps, s->f32, s->n, c, sw)));
        g_sweeps_launched++;
    }
    return QSIM_OK;
}

// checked arguments; C may be NULL: no controls anywhere
static int apply_rotations(qsim_state *s, const uint64_t *C, const uint64_t *X, const uint64_t *Z, const double *thetas, long num) {
    for (const RotRoute &r : route_rotations(X, Z, num, index_mask(s->n), C)) {
        const uint64_t c = C ? C[r.first] : 0, x = X[r.first];
        if (r.gate) {
            const bool y = (Z[r.first] & x) != 0;
            const int target = __builtin_ctzll(x), control = c ? __builtin_ctzll(c) : -1;
            double U[32];
            if (c) {
                controlled_rot_2q(y, thetas[r.first], control > target, U);
                QSIM_TRY(qsim_apply_2q(s, U, std::max(control, target), std::min(control, target)));
            } else {
                pauli_rot_1q(y, thetas[r.first], U);
                QSIM_TRY(qsim_apply_1q(s, U, target));
            }
        } else if (c) {
            QSIM_TRY(controlled_rot_run(s, c, x, Z + r.first, thetas + r.first, r.count));
        } else {
            QSIM_TRY(pauli_rot_run(s, nullptr, 0, x, Z + r.first, thetas + r.first, r.count));
        }
    }
    return QSIM_OK;
}

extern "C" int qsim_apply_pauli_rotations(qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, const double *thetas, long num_terms) {
    QSIM_TRY(check_terms("qsim_apply_pauli_rotations", s, x_masks, z_masks, thetas, thetas, num_terms));
    return apply_rotations(s, nullptr, x_masks, z_masks, thetas, num_terms);
}

extern "C" int qsim_apply_controlled_pauli_rotations(qsim_state *s, const uint64_t *c_masks, const uint64_t *x_masks, const uint64_t *z_masks,
                                                     const double *thetas, long num_terms) {
    const char *who = "qsim_apply_controlled_pauli_rotations";
    QSIM_TRY(check_terms(who, s, x_masks, z_masks, thetas, thetas, num_terms));
    QSIM_TRY(check_controls(who, s->n, c_masks, x_masks, z_masks, num_terms));
    return apply_rotations(s, c_masks, x_masks, z_masks, thetas, num_terms);
}

extern "C" int qsim_controlled_rotation_plan(const uint64_t *c_masks, const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, int num_q,
                                             int precision_bits, long *sweeps, long *queued_as_gates, uint64_t *units_visited) {
    const char *who = "qsim_controlled_rotation_plan";
    if (!sweeps || !queued_as_gates || !units_visited) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    QSIM_TRY(check_pauli_terms(fail, who, num_q, x_masks, z_masks, x_masks, nullptr, num_terms));
    QSIM_TRY(check_controls(who, num_q, c_masks, x_masks, z_masks, num_terms));
    *sweeps = *queued_as_gates = 0;
    *units_visited = 0;
    const bool f32 = precision_bits == 32;
    for (const RotRoute &r : route_rotations(x_masks, z_masks, num_terms, index_mask(num_q), c_masks)) {
        if (r.gate) {
            ++*queued_as_gates;
            continue;
        }
        const uint64_t c = c_masks ? c_masks[r.first] : 0, x = x_masks[r.first];
        *sweeps += rotation_sweeps(r.count);
        *units_visited += (uint64_t)rotation_sweeps(r.count) * (c ? ctrl_geom(c, x, f32, num_q).units : sweep_geom(x, false, f32, num_q).units);
    }
    return QSIM_OK;
}

// ---- adjoint gradients ------------------------------------------------------------------------------------------------------------
// E = <psi_K|H|psi_K> and dE/dtheta_k = Im <lambda_k|P_k|psi_k> (adjoint.hip has the pair formula): forward pass, lambda = H psi,
// energy, then the backward sweeps over psi and lambda, which also take the state back to where the call found it.
static std::atomic<uint64_t> g_adjoint_sweeps{0};
extern "C" uint64_t qsim_pauli_adjoint_sweeps_launched(void) { return g_adjoint_sweeps.load(); }
static std::atomic<uint64_t> g_diag_adjoint_sweeps{0}; // the backward sweeps through diagonal phases, which count here only
extern "C" uint64_t qsim_diagonal_adjoint_sweeps_launched(void) { return g_diag_adjoint_sweeps.load(); }

// The backward sweeps in FORWARD order: maximal runs of consecutive equal x and equal control mask (C may be NULL: no controls
// anywhere), cut into pieces of K.  Every term, single X and Y too.  A step that is a diagonal phase (diag(t): DESIGN §7k) is a piece
// of its own, and no run fuses across it; its x and control mask are not looked at.
template <typename IsDiag>
static std::vector<std::pair<long, int>> adjoint_pieces(const uint64_t *C, const uint64_t *X, long num, IsDiag diag) {
    std::vector<std::pair<long, int>> out;
    auto c = [&](long t) { return C ? C[t] : 0; };
    for (long t = 0; t < num;) {
        if (diag(t)) {
            out.emplace_back(t++, 1);
            continue;
        }
        long e = t + 1;
        while (e < num && !diag(e) && X[e] == X[t] && c(e) == c(t)) e++;
        for (; t < e; t += kPauliRotationsPerSweep) out.emplace_back(t, (int)std::min<long>(kPauliRotationsPerSweep, e - t));
        t = e;
    }
    return out;
}
static std::vector<std::pair<long, int>> adjoint_pieces(const uint64_t *C, const uint64_t *X, long num) {
    return adjoint_pieces(C, X, num, [](long) { return false; });
}

extern "C" int qsim_pauli_gradient_plan(const uint64_t *rot_x, long num_rot, const uint64_t *ham_x, long num_ham, long *adjoint_sweeps, long *sum_sweeps) {
    if (num_rot < 0 || num_ham < 0) return fail(QSIM_ERR_ARG, "qsim_pauli_gradient_plan: negative term count");
    if (!adjoint_sweeps || !sum_sweeps || (num_rot > 0 && !rot_x) || (num_ham > 0 && !ham_x)) return fail(QSIM_ERR_ARG, "qsim_pauli_gradient_plan: NULL argument");
    *adjoint_sweeps = (long)adjoint_pieces(nullptr, rot_x, num_rot).size();
    *sum_sweeps = (long)pauli_sweeps(ham_x, ~0ULL, num_ham).sweeps.size();
    return QSIM_OK;
}

extern "C" int qsim_controlled_gradient_plan(const uint64_t *rot_c, const uint64_t *rot_x, long num_rot, const uint64_t *ham_x, long num_ham, int num_q,
                                             int precision_bits, long *adjoint_sweeps, long *sum_sweeps, uint64_t *units_visited) {
    const char *who = "qsim_controlled_gradient_plan";
    if (!adjoint_sweeps || !sum_sweeps || !units_visited) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    // the plan knows no z: x stands in for it, so a control that meets x is refused here and one that meets z by the call itself
    QSIM_TRY(check_pauli_terms(fail, who, num_q, rot_x, rot_x, rot_x, nullptr, num_rot));
    QSIM_TRY(check_pauli_terms(fail, who, num_q, ham_x, ham_x, ham_x, nullptr, num_ham));
    QSIM_TRY(check_controls(who, num_q, rot_c, rot_x, rot_x, num_rot));
    const bool f32 = precision_bits == 32;
    const std::vector<std::pair<long, int>> pieces = adjoint_pieces(rot_c, rot_x, num_rot);
    *adjoint_sweeps = (long)pieces.size();
    *sum_sweeps = (long)pauli_sweeps(ham_x, ~0ULL, num_ham).sweeps.size();
    *units_visited = 0;
    for (const std::pair<long, int> &piece : pieces) { // one unit index addresses psi and lambda
        const uint64_t c = rot_c ? rot_c[piece.first] : 0, x = rot_x[piece.first];
        *units_visited += c ? ctrl_geom(c, x, f32, num_q).units : sweep_geom(x, false, f32, num_q).units;
    }
    return QSIM_OK;
}

// dst = sum_t C[t] Q_t |state> for a settled state and checked arguments: one sweep per piece of an x group, the first stores.
int qsim::pauli_sum_sweeps(qsim_state *s, const uint64_t *X, const uint64_t *Z, const double *C, long num, void *dst) {
    if (num == 0) { // the empty sum
        HIP_TRY(hipMemsetAsync(dst, 0, s->amp_bytes() << s->n, s->stream));
        return QSIM_OK;
    }
    const PauliSweeps plan = pauli_sweeps(X, ~0ULL, num);
    const LaunchCfg cfg{s->stream, s->grid_cap};
    for (size_t w = 0; w < plan.sweeps.size(); w++) {
        SumSweep sw{};
        sw.x = X[plan.order[(size_t)plan.sweeps[w].first]];
        sw.count = plan.sweeps[w].second;
        sw.accumulate = w > 0;
        for (int k = 0; k < sw.count; k++) {
            const long t = plan.order[(size_t)(plan.sweeps[w].first + k)];
            const int ny = __builtin_popcountll(X[t] & Z[t]);
            sw.z[k] = Z[t];
            sw.c[k] = C[t] * pauli_phase(ny) * ((ny & 1) ? -1.0 : 1.0); // (Q psi)_i = i^ny s(i ^ x) psi_(i^x), and s(i ^ x) = (-1)^ny s(i)
            if (ny & 1) sw.odd_mask |= 1u << k;
        }
        QSIM_TRY(launched("Pauli sum sweep", launch_pauli_sum(cfg, s->amps, dst, s->f32, s->n, sw)));
    }
    return QSIM_OK;
}

extern "C" int qsim_pauli_sum_into(qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, const double *coeffs, long num_terms, void *dst_device) {
    QSIM_TRY(check_terms("qsim_pauli_sum_into", s, x_masks, z_masks, coeffs, coeffs, num_terms, "coefficient"));
    QSIM_TRY(await_buffer(s));
    if (!dst_device || dst_device == s->amps || dst_device == s->spare)
        return fail(QSIM_ERR_ARG, "qsim_pauli_sum_into: the destination is NULL or one of the state's own buffers");
    QSIM_TRY(settle(s));
    return pauli_sum_sweeps(s, x_masks, z_masks, coeffs, num_terms, dst_device);
}

// The diagonal parts of a gradient call: step k of the circuit is exp(-i thetas[k] D) where step[k] is a table (NULL
// array: no such step; the step's c, x and z are not looked at), and H has the part weight * D_obs (obs NULL: none).
struct GradientDiagonals {
    const qsim_diagonal *const *step = nullptr;
    const qsim_diagonal *obs = nullptr;
    double weight = 0.0;
    const qsim_diagonal *at(long t) const { return step ? step[t] : nullptr; }
};

// checked arguments; C may be NULL: no controls anywhere.  The ONE owner of the adjoint algorithm: without diagonal parts its forward
// loop is one apply_rotations call over the whole list and its pieces are the rotations' alone, which is what qsim_pauli_gradient and
// qsim_controlled_pauli_gradient run.
static int gradient(qsim_state *s, const uint64_t *C, const uint64_t *rot_x, const uint64_t *rot_z, const double *thetas, long num_rot, const uint64_t *ham_x,
                    const uint64_t *ham_z, const double *coeffs, long num_ham, double *energy, double *grad, const GradientDiagonals &dg = {}) {
    if (energy) *energy = 0.0;
    if (grad) std::fill(grad, grad + num_rot, 0.0);
    if (qsim_holds_nothing(s)) return QSIM_OK; // the zero vector: energy 0, gradient 0, no sweep
    QSIM_TRY(await_buffer(s));
    HIP_TRY(hipSetDevice(s->device));
    // everything that can fail for want of memory comes before the state is touched
    void *lam = nullptr;
    QSIM_TRY(second_buffer(s, &lam));
    QSIM_TRY(alloc_sweep_scratch(s));
    const LaunchCfg cfg{s->stream, s->grid_cap};

    // forward: the runs of rotations between the diagonal steps as apply_rotations takes them; a diagonal step is one phase sweep
    for (long t = 0; t < num_rot;) {
        long e = t;
        while (e < num_rot && !dg.at(e)) e++;
        if (e > t) QSIM_TRY(apply_rotations(s, C ? C + t : nullptr, rot_x + t, rot_z + t, thetas + t, e - t));
        if (e < num_rot) {
            QSIM_TRY(settle(s)); // single X and Y rotations wait in the gate queue
            QSIM_TRY(launched("diagonal phase sweep", launch_diag_phase(cfg, s->amps, s->f32, s->n, diag_table(dg.at(e)), thetas[e] / M_PI)));
            count_diagonal_sweep();
            QSIM_TRY(mark_read(s, dg.at(e)));
            e++;
        }
        t = e;
    }
    QSIM_TRY(settle(s));
    // lambda = H psi: the Pauli part stores (zeros when there is none and no diagonal part either), the diagonal part comes on top
    if (num_ham > 0 || !dg.obs) QSIM_TRY(pauli_sum_sweeps(s, ham_x, ham_z, coeffs, num_ham, lam));
    if (dg.obs) {
        QSIM_TRY(launched("diagonal sum sweep", launch_diag_apply(cfg, s->amps, lam, s->f32, s->n, diag_table(dg.obs), dg.weight, num_ham > 0)));
        count_diagonal_sweep();
        QSIM_TRY(mark_read(s, dg.obs));
    }

    // row 0: the energy, Re <lambda|psi>, as one paired expectation sweep over the two buffers; then the pieces, last first
    const std::vector<std::pair<long, int>> pieces = adjoint_pieces(C, rot_x, num_rot, [&](long t) { return dg.at(t) != nullptr; });
    return sweep_result_rows(
        s, 1 + pieces.size(),
        [&](size_t r, double *d_row) -> int {
            if (r == 0) {
                ExpectSweep sw{};
                sw.full = true; // x == 0 over two buffers: every index, its partner the same index of lambda
                sw.count = 1;
                return launched("expectation sweep", launch_expect(cfg, s->amps, lam, s->f32, s->n, sw, sweep_partials(s), d_row));
            }
            const std::pair<long, int> &piece = pieces[pieces.size() - r];
            if (const qsim_diagonal *d = dg.at(piece.first)) { // the step back is the phase of -gamma
                QSIM_TRY(launched("diagonal adjoint sweep",
                                  launch_diag_adjoint(cfg, s->amps, lam, s->f32, s->n, diag_table(d), -thetas[piece.first] / M_PI, sweep_partials(s), d_row)));
                g_diag_adjoint_sweeps++;
                return mark_read(s, d);
            }
            const uint64_t c = C ? C[piece.first] : 0;
            const RotSweep sw = rot_sweep(rot_x[piece.first], rot_z + piece.first, thetas + piece.first, piece.second, -1.0 /* U^+ */, 0, index_mask(s->n), s->n);
            if (c) QSIM_TRY(launched("controlled adjoint sweep", launch_pauli_cadjoint(cfg, s->amps, lam, s->f32, s->n, c, sw, sweep_partials(s), d_row)));
            else QSIM_TRY(launched("adjoint sweep", launch_pauli_adjoint(cfg, s->amps, lam, s->f32, s->n, sw, sweep_partials(s), d_row)));
            g_adjoint_sweeps++;
            return QSIM_OK;
        },
        [&](size_t r, const double *row) {
            if (r == 0) {
                if (energy) *energy = row[0];
                return;
            }
            const std::pair<long, int> &piece = pieces[pieces.size() - r];
            if (dg.at(piece.first)) { // dE/dgamma = 2 Re <lambda|(-i) D|psi> = 2 sum_i d_i Im(conj(lambda_i) psi_i)
                if (grad) grad[piece.first] = 2.0 * row[0];
                return;
            }
            // Im (i^ny B): the kernel summed Im B (even ny) or Re B (odd); both members of a pair are in B, so the factor is 1, not 2
            for (int k = 0; grad && k < piece.second; k++)
                grad[piece.first + k] = pauli_phase(__builtin_popcountll(rot_x[piece.first] & rot_z[piece.first + k])) * row[k];
        });
}

extern "C" int qsim_pauli_gradient(qsim_state *s, const uint64_t *rot_x, const uint64_t *rot_z, const double *thetas, long num_rot,
                                   const uint64_t *ham_x, const uint64_t *ham_z, const double *coeffs, long num_ham, double *energy, double *grad) {
    QSIM_TRY(check_terms("qsim_pauli_gradient", s, rot_x, rot_z, thetas, thetas, num_rot));
    QSIM_TRY(check_terms("qsim_pauli_gradient", s, ham_x, ham_z, coeffs, coeffs, num_ham, "coefficient"));
    return gradient(s, nullptr, rot_x, rot_z, thetas, num_rot, ham_x, ham_z, coeffs, num_ham, energy, grad);
}

// The same through controlled rotations (cadjoint.hip; DESIGN "Adjoint gradients under controls"): dE/dtheta_k = Im <lambda_k|Pi_k P_k|psi_k>,
// the pair bracket inside the control subspace, where alone U_k^+ steps psi and lambda back.
extern "C" int qsim_controlled_pauli_gradient(qsim_state *s, const uint64_t *rot_c, const uint64_t *rot_x, const uint64_t *rot_z, const double *thetas,
                                              long num_rot, const uint64_t *ham_x, const uint64_t *ham_z, const double *coeffs, long num_ham, double *energy,
                                              double *grad) {
    const char *who = "qsim_controlled_pauli_gradient";
    QSIM_TRY(check_terms(who, s, rot_x, rot_z, thetas, thetas, num_rot));
    QSIM_TRY(check_terms(who, s, ham_x, ham_z, coeffs, coeffs, num_ham, "coefficient"));
    QSIM_TRY(check_controls(who, s->n, rot_c, rot_x, rot_z, num_rot));
    return gradient(s, rot_c, rot_x, rot_z, thetas, num_rot, ham_x, ham_z, coeffs, num_ham, energy, grad);
}

// ---- the same through diagonal phases, and with a diagonal part of H (diagonal.hip) --------------------------------------
// What both the call and its plan check of a mixed step list: every rotation step by check_pauli_terms and check_controls, one step
// at a time, so that what is refused has one definition (Z NULL: the plan, which knows no z, x stands in; angles NULL: the plan), and
// on a diagonal step a finite gamma and no control mask.  diag(t): step t is diagonal.
template <typename IsDiag>
static int check_steps(const char *who, int n, IsDiag diag, const uint64_t *C, const uint64_t *X, const uint64_t *Z, const double *angles, bool plan, long num) {
    if (num < 0) return fail(QSIM_ERR_ARG, "%s: negative step count", who);
    for (long t = 0; t < num; t++) {
        if (diag(t)) {
            if (angles && !std::isfinite(angles[t])) return fail(QSIM_ERR_ARG, "%s: term %ld has a non-finite gamma", who, t);
            if (C && C[t]) return fail(QSIM_ERR_ARG, "%s: term %ld is a diagonal phase and carries a control mask", who, t);
            continue;
        }
        const uint64_t *x = X ? X + t : nullptr, *z = plan ? x : Z ? Z + t : nullptr;
        QSIM_TRY(check_pauli_terms(fail, who, n, x, z, plan ? (const void *)x : (const void *)angles, plan ? nullptr : angles + t, 1, "angle", t));
        QSIM_TRY(check_controls(who, n, C ? C + t : nullptr, x, z, 1, t));
    }
    return QSIM_OK;
}

extern "C" int qsim_diagonal_gradient(qsim_state *s, long num_steps, const qsim_diagonal *const *step_diag, const uint64_t *step_c, const uint64_t *step_x,
                                      const uint64_t *step_z, const double *angles, const uint64_t *ham_x, const uint64_t *ham_z, const double *coeffs,
                                      long num_ham, const qsim_diagonal *obs, double obs_weight, double *energy, double *grad) {
    const char *who = "qsim_diagonal_gradient";
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    if (num_steps > 0 && !angles) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    GradientDiagonals dg;
    dg.step = step_diag;
    QSIM_TRY(check_steps(who, s->n, [&](long t) { return dg.at(t) != nullptr; }, step_c, step_x, step_z, angles, false, num_steps));
    for (long t = 0; t < num_steps; t++)
        if (dg.at(t)) QSIM_TRY(check_diag_pair(who, s, dg.at(t)));
    QSIM_TRY(check_terms(who, s, ham_x, ham_z, coeffs, coeffs, num_ham, "coefficient"));
    if (obs) {
        QSIM_TRY(check_diag_pair(who, s, obs));
        if (!std::isfinite(obs_weight)) return fail(QSIM_ERR_ARG, "%s: a non-finite weight of the diagonal part", who);
        dg.obs = obs, dg.weight = obs_weight;
    }
    return gradient(s, step_c, step_x, step_z, angles, num_steps, ham_x, ham_z, coeffs, num_ham, energy, grad, dg);
}

extern "C" int qsim_diagonal_gradient_plan(const unsigned char *is_diag, const uint64_t *step_c, const uint64_t *step_x, long num_steps, const uint64_t *ham_x,
                                           long num_ham, int has_obs, int num_q, int precision_bits, long *pauli_adjoint_sweeps, long *diag_adjoint_sweeps,
                                           long *sum_sweeps, int *diag_adjoint_items_per_trip, long *diag_adjoint_trips_at_cap) {
    const char *who = "qsim_diagonal_gradient_plan";
    if (!pauli_adjoint_sweeps || !diag_adjoint_sweeps || !sum_sweeps || !diag_adjoint_items_per_trip || !diag_adjoint_trips_at_cap)
        return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    auto diag = [&](long t) { return is_diag && is_diag[t] != 0; };
    QSIM_TRY(check_steps(who, num_q, diag, step_c, step_x, nullptr, nullptr, true, num_steps));
    QSIM_TRY(check_pauli_terms(fail, who, num_q, ham_x, ham_x, ham_x, nullptr, num_ham));
    *pauli_adjoint_sweeps = *diag_adjoint_sweeps = 0;
    for (const std::pair<long, int> &piece : adjoint_pieces(step_c, step_x, num_steps, diag)) ++*(diag(piece.first) ? diag_adjoint_sweeps : pauli_adjoint_sweeps);
    *sum_sweeps = (long)pauli_sweeps(ham_x, ~0ULL, num_ham).sweeps.size() + (has_obs ? 1 : 0);
    const DiagGeom g = diag_geom(num_q);
    *diag_adjoint_items_per_trip = qsim::diag_adjoint_items_per_trip(precision_bits == 32);
    const uint64_t blocks = (g.items + kTPB - 1) / kTPB;
    *diag_adjoint_trips_at_cap = g.items < (uint64_t)kDiagWave ? 1 : trips_at_cap(blocks, (uint64_t)*diag_adjoint_items_per_trip, kExpectGrid);
    return QSIM_OK;
}
