// matrix.cpp — dense matrices on up to five target qubits under controls: the plan (the one place that decides the path, the
// padding, the shape and the geometry), the operand the kernel is handed, and the entry points.  The kernels are
// matrix.hip's; matrix.h has the decomposition they share with this file.  The call settles the state, launches one in-place sweep of
// the control subspace on the state's stream and returns without waiting: the coefficients travel through a pinned staging ring to
// the state's sweep scratch, both stream-ordered.
#include <atomic>
#include <cmath>
#include <complex>
#include <cstring>
#include <map>
#include <mutex>

#include "engine_state.h"
#include "matrix.h"

using namespace qsim;
using cplx = std::complex<double>;

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
bool qsim::matrix_plan(const int *targets, int k, const int *controls, int num_controls, int n, bool f32, MatrixPlan *out) {
    uint64_t mask, cmask;
    if (n < 0 || n > 40 || k > kMatrixMaxQubits) return false;
    if (!qubit_list_mask(targets, k, n, 0, &mask) || !qubit_list_mask(controls, num_controls, n, mask, &cmask)) return false;
    MatrixPlan p{};
    std::copy(targets, targets + k, p.targets);
    p.n = n, p.k = k, p.num_controls = num_controls, p.f32 = f32, p.controls = cmask;
    const bool q0_ctrl = f32 && (cmask & 1ULL);
    p.units = ((1ULL << n) >> num_controls) >> (f32 && !q0_ctrl ? 1 : 0);
    if (p.units == 0) p.units = 1; // one active fp32 amplitude
    // the matrix path: a subset of 3 to 5 qubits, padded with the lowest bits that are free, and 16 environment units per instruction
    const int kk = k < kMatrixMinKernelQubits ? kMatrixMinKernelQubits : k;
    const uint64_t padded = pad_subset(mask, cmask, kk, n);
    p.path = 0;
    if (__builtin_popcountll(padded) == kk) {
        const uint64_t env_units = matrix_geom(padded, cmask, f32, n).units;
        if (env_units >= (uint64_t)kMatrixEnvsPerStep) p.path = 1, p.env_units = env_units;
    }
    p.padded_k = p.path ? kk : k;
    p.mask = p.path ? padded : mask;
    p.mode = !f32 || (p.mask & 1ULL) ? kMatrixRows : q0_ctrl ? kMatrixCtrl : kMatrixEnvs;
    p.trips_at_cap = 1;
    if (p.path) {
        const uint64_t per_trip = (uint64_t)kMatrixWaves * matrix_steps_per_trip(matrix_lane_units(f32, kk, p.mode));
        p.trips_at_cap = trips_at_cap(p.env_units >> 4, per_trip, matrix_grid_cap(kk));
    }
    *out = p;
    return true;
}

// ---- the operand ------------------------------------------------------------------------------------------------------------------
// U (x) 1 over the plan's sorted subset: 2^padded_k square; bit j of a row or column index of U is qubit targets[j]
static std::vector<cplx> padded_matrix(const MatrixPlan &p, const double *U) {
    const int kdim = 1 << p.padded_k, dim = 1 << p.k;
    const SubsetOrder order{p.mask, p.targets, p.k};
    const uint32_t own = order.own();
    std::vector<cplx> out((size_t)kdim * kdim, cplx(0.0, 0.0));
    for (uint32_t a = 0; a < (uint32_t)kdim; a++)
        for (uint32_t b = 0; b < (uint32_t)kdim; b++)
            if (((a ^ b) & ~own) == 0) { // the identity on the padding
                const size_t at = (size_t)order.to_callers(a) * dim + order.to_callers(b);
                out[(size_t)a * kdim + b] = cplx(U[2 * at], U[2 * at + 1]);
            }
    return out;
}

// M = [[Re U, -Im U], [Im U, Re U]] of the padded matrix, rows and columns in the kernel's order (matrix_row), row-major
static std::vector<double> real_operand(const MatrixPlan &p, const double *U, std::vector<int> *row_amp = nullptr, std::vector<int> *row_part = nullptr) {
    const int rows = matrix_rows(p.padded_k), kdim = 1 << p.padded_k;
    const std::vector<cplx> up = padded_matrix(p, U);
    std::vector<int> amp(rows), part(rows);
    for (int r = 0; r < rows; r++) matrix_row(p.f32, p.mode, r, &amp[r], &part[r]);
    std::vector<double> M((size_t)rows * rows);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < rows; c++) {
            const cplx u = up[(size_t)amp[r] * kdim + amp[c]];
            M[(size_t)r * rows + c] = part[r] == part[c] ? u.real() : part[r] ? u.imag() : -u.imag();
        }
    if (row_amp) *row_amp = amp;
    if (row_part) *row_part = part;
    return M;
}

static int to_plan(const char *who, const int *targets, int k, const int *controls, int num_controls, int n, bool f32, MatrixPlan *p) {
    if (!matrix_plan(targets, k, controls, num_controls, n, f32, p))
        return fail(QSIM_ERR_ARG, "%s: 0 to %d distinct target qubits and any number of distinct control qubits, disjoint, inside the register of %d", who,
                    kMatrixMaxQubits, n);
    return QSIM_OK;
}

static bool all_finite(const double *U, int k) {
    for (size_t i = 0; i < ((size_t)2 << (2 * k)); i++)
        if (!std::isfinite(U[i])) return false;
    return true;
}

extern "C" int qsim_apply_matrix_max_qubits(void) { return kMatrixMaxQubits; }

extern "C" int qsim_apply_matrix_plan(const int *targets, int k, const int *controls, int num_controls, int num_q, int precision_bits, int *path,
                                      int *padded_k, uint64_t *kernel_mask, uint64_t *units, long *trips_per_workgroup) {
    const char *who = "qsim_apply_matrix_plan";
    if (!path || !padded_k || !kernel_mask || !units || !trips_per_workgroup) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    MatrixPlan p;
    QSIM_TRY(to_plan(who, targets, k, controls, num_controls, num_q, precision_bits == 32, &p));
    subset_probe_outputs(p, path, padded_k, kernel_mask, units, trips_per_workgroup);
    return QSIM_OK;
}

extern "C" int qsim_apply_matrix_operand(const double *U, const int *targets, int k, const int *controls, int num_controls, int num_q,
                                         int precision_bits, double *M, int *row_amp, int *row_part, int *rows) {
    const char *who = "qsim_apply_matrix_operand";
    if (!U || !M || !row_amp || !row_part || !rows) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    MatrixPlan p;
    QSIM_TRY(to_plan(who, targets, k, controls, num_controls, num_q, precision_bits == 32, &p));
    if (!all_finite(U, k)) return fail(QSIM_ERR_ARG, "%s: a non-finite matrix entry", who);
    *rows = 0;
    if (!p.path) return QSIM_OK; // the plain kernel takes U as it is
    std::vector<int> amp, part;
    const std::vector<double> m = real_operand(p, U, &amp, &part);
    *rows = matrix_rows(p.padded_k);
    std::copy(m.begin(), m.end(), M);
    std::copy(amp.begin(), amp.end(), row_amp);
    std::copy(part.begin(), part.end(), row_part);
    return QSIM_OK;
}

// ---- the way of the coefficients to the device --------------------------------------------------------------------------------------
// A ring of pinned slots per device.  A slot is free again when the copy out of it has run (its event), so a call waits only when
// kSlots calls of one device are still queued; the copy itself is ordered on the state's stream, in front of the sweep.
// qsim_apply_permutation (permutation.cpp) sends its destination map the same way.
namespace {
constexpr int kSlots = 16;
struct Ring {
    double *host = nullptr;
    hipEvent_t done[kSlots] = {};
    hipStream_t on[kSlots] = {}; // the stream `done` was last recorded on
    bool used[kSlots] = {};
    int next = 0;
};
std::mutex g_ring_mutex;
std::map<int, Ring> g_rings;
} // namespace

int qsim::stage_sweep_operand(qsim_state *s, const void *data, size_t bytes) {
    if (bytes > kMatrixCoefDoubles * sizeof(double)) return fail(QSIM_ERR_ARG, "stage_sweep_operand: %zu bytes do not fit a slot", bytes);
    QSIM_TRY(alloc_sweep_scratch(s)); // stream-ordered scratch of the state's own
    std::lock_guard<std::mutex> lock(g_ring_mutex);
    Ring &ring = g_rings[s->device];
    if (!ring.host) {
        HIP_TRY(hipHostMalloc((void **)&ring.host, kSlots * kMatrixCoefDoubles * sizeof(double), hipHostMallocDefault));
        for (int i = 0; i < kSlots; i++) HIP_TRY(hipEventCreateWithFlags(&ring.done[i], hipEventDisableTiming));
    }
    const int slot = ring.next;
    ring.next = (slot + 1) % kSlots;
    if (ring.used[slot]) HIP_TRY(hipEventSynchronize(ring.done[slot]));
    double *h = ring.host + (size_t)slot * kMatrixCoefDoubles;
    std::memcpy(h, data, bytes);
    HIP_TRY(hipMemcpyAsync(sweep_coef_staging(s), h, bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(ring.done[slot], s->stream));
    ring.on[slot] = s->stream;
    ring.used[slot] = true;
    return QSIM_OK;
}

void qsim::forget_staged_operands(const qsim_state *s) {
    std::lock_guard<std::mutex> lock(g_ring_mutex);
    const auto it = g_rings.find(s->device);
    if (it == g_rings.end()) return;
    for (int i = 0; i < kSlots; i++)
        if (it->second.on[i] == s->stream) it->second.used[i] = false;
}

// ---- the call ---------------------------------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_matrix_sweeps{0};
extern "C" uint64_t qsim_matrix_sweeps_launched(void) { return g_matrix_sweeps.load(); }

extern "C" int qsim_apply_matrix(qsim_state *s, const double *U, const int *targets, int k, const int *controls, int num_controls) {
    const char *who = "qsim_apply_matrix";
    if (!s || !U) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    MatrixPlan p;
    QSIM_TRY(to_plan(who, targets, k, controls, num_controls, s->n, s->f32, &p));
    if (!all_finite(U, k)) return fail(QSIM_ERR_ARG, "%s: a non-finite matrix entry", who);
    if (qsim_holds_nothing(s)) return QSIM_OK; // the zero vector stays the zero vector
    QSIM_TRY(await_buffer(s));
    QSIM_TRY(settle(s));
    std::vector<double> coef;
    if (p.path) { // M, lane-major: what a lane keeps in registers for (result tile t, slice s)
        const int rows = matrix_rows(p.padded_k), tiles = matrix_tiles(p.padded_k), slices = matrix_slices(p.padded_k);
        const std::vector<double> m = real_operand(p, U);
        coef.resize((size_t)rows * rows);
        for (int t = 0; t < tiles; t++)
            for (int sl = 0; sl < slices; sl++)
                for (int lane = 0; lane < 64; lane++)
                    coef[matrix_coef_index(p.padded_k, t, sl, lane)] = m[(size_t)(16 * t + (lane & 15)) * rows + 4 * sl + (lane >> 4)];
    } else {
        coef.assign(U, U + ((size_t)2 << (2 * k)));
    }
    QSIM_TRY(stage_sweep_operand(s, coef.data(), coef.size() * sizeof(double)));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    QSIM_TRY(launched("qsim_apply_matrix:", launch_matrix(cfg, s->amps, p, sweep_coef_staging(s))));
    g_matrix_sweeps++;
    return QSIM_OK;
}
