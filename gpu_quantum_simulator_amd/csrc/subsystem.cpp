// subsystem.cpp — reduced density matrices of 6 to 10 qubits: the plan (the one place that decides the path, the blocks and the
// slices), the entry points, and the way back from the result blocks to rho in the caller's qubit order.  The kernels
// are subsystem.hip's; subsystem.h has the decomposition they share with this file.  Read-only: the call settles the state, reads it
// and writes nothing but its own scratch, which is allocated per call before anything is launched.  Five qubits and fewer are
// forwarded to qsim_reduced_density and return its bits.
#include <atomic>
#include <complex>

#include "engine_state.h"
#include "subsystem.h"

using namespace qsim;

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
bool qsim::subsystem_plan(const int *qubits, int k, int n, bool f32, SubsystemPlan *out) {
    uint64_t mask;
    if (n < 0 || n > 40 || k > kSubsystemMaxQubits || !qubit_list_mask(qubits, k, n, 0, &mask)) return false;
    SubsystemPlan p{};
    p.n = n, p.k = k, p.f32 = f32, p.mask = mask;
    p.trips = 1;
    const int as = f32 ? 1 : 0;
    if (k < kSubsystemMinQubits) { // qsim_reduced_density's: qsim_reduced_density_plan says what it does
        p.path = 2;
        p.units_read = std::max<uint64_t>((1ULL << n) >> as, 1);
    } else if (n - k < 2) {
        p.path = 0;
        p.units_read = (2ULL << (2 * k + (n - k))) >> as; // every element reads two amplitudes per environment
        p.scratch_bytes = 16ULL << (2 * k);
    } else {
        p.path = 1;
        p.block_rows = kSubBlockRows;
        p.blocks = (2L << k) / kSubBlockRows;
        p.upper_blocks = p.blocks * (p.blocks + 1) / 2;
        p.chunk_env_bits = std::min(kSubChunkEnvBits, n - k);
        p.chunks = 1L << (n - k - p.chunk_env_bits);
        long target = 1; // the largest power of two with target * upper_blocks <= kSubMaxPartialBlocks, kSubMaxSlices at most
        while (2 * target * p.upper_blocks <= kSubMaxPartialBlocks && 2 * target <= kSubMaxSlices) target *= 2;
        p.slices = std::min(target, std::max(1L, p.chunks / kSubMinTrips));
        p.trips = p.chunks / p.slices;
        p.units_read = ((1ULL << n) >> as) * (uint64_t)p.blocks; // an off-diagonal block reads two panels, a diagonal one its own
        p.scratch_bytes = (uint64_t)(p.slices + 1) * p.upper_blocks * kSubBlockDoubles * sizeof(double);
    }
    *out = p;
    return true;
}

extern "C" int qsim_subsystem_density_max_qubits(void) { return kSubsystemMaxQubits; }

extern "C" int qsim_subsystem_density_plan(const int *qubits, int k, int num_q, int precision_bits, int *path, int *block_rows, long *upper_blocks,
                                           long *slices, uint64_t *units_read, uint64_t *scratch_bytes, long *trips_per_workgroup) {
    const char *who = "qsim_subsystem_density_plan";
    if (!path || !block_rows || !upper_blocks || !slices || !units_read || !scratch_bytes || !trips_per_workgroup)
        return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    SubsystemPlan p;
    if (!subsystem_plan(qubits, k, num_q, precision_bits == 32, &p))
        return fail(QSIM_ERR_ARG, "%s: 0 to %d distinct qubits inside the register, not more than it has", who, kSubsystemMaxQubits);
    *path = p.path, *block_rows = p.block_rows, *upper_blocks = p.upper_blocks, *slices = p.slices, *units_read = p.units_read;
    *scratch_bytes = p.scratch_bytes, *trips_per_workgroup = p.trips;
    return QSIM_OK;
}

// ---- from the result blocks to rho ----------------------------------------------------------------------------------------------------
using cplx = std::complex<double>;

// rho over the sorted subset, Hermitian bit for bit, from the upper blocks of G: row 2 a of R is Re Psi[a], row 2 a + 1 Im Psi[a];
// Re rho = G_RR + G_II, Im rho = G_IR - G_RI for a <= b, the lower triangle its conjugate, the diagonal real.
static std::vector<cplx> rho_from_blocks(const SubsystemPlan &p, const double *g) {
    const size_t dim = (size_t)1 << p.k;
    const int half = kSubBlockRows / 2;
    std::vector<cplx> rho(dim * dim);
    for (size_t a = 0; a < dim; a++)
        for (size_t b = a; b < dim; b++) {
            const double *blk = g + (size_t)subsystem_block_index(p.blocks, (long)(a / half), (long)(b / half)) * kSubBlockDoubles;
            const size_t r = 2 * (a % half), c = 2 * (b % half);
            auto G = [&](size_t pr, size_t pc) { return blk[(r + pr) * kSubBlockRows + c + pc]; };
            const cplx v(G(0, 0) + G(1, 1), a == b ? 0.0 : G(1, 0) - G(0, 1));
            rho[a * dim + b] = v;
            rho[b * dim + a] = std::conj(v);
        }
    for (size_t a = 0; a < dim; a++) rho[a * dim + a] = cplx(rho[a * dim + a].real(), 0.0); // not -0
    return rho;
}

// out = rho in the caller's qubit order: bit j of an index is qubit qubits[j].  A permutation of rows and columns alike: Hermitian
// stays Hermitian, bit for bit.
static void to_callers_order(const SubsystemPlan &p, const int *qubits, const std::vector<cplx> &rho, double *out) {
    const size_t dim = (size_t)1 << p.k;
    const SubsetOrder order{p.mask, qubits, p.k};
    std::vector<uint32_t> at(dim);
    for (size_t c = 0; c < dim; c++) at[c] = order.to_subset((uint32_t)c);
    for (size_t a = 0; a < dim; a++)
        for (size_t b = 0; b < dim; b++) {
            const cplx v = rho[(size_t)at[a] * dim + at[b]];
            out[2 * (a * dim + b)] = v.real(), out[2 * (a * dim + b) + 1] = v.imag();
        }
}

// ---- the call ---------------------------------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_subsystem_sweeps{0};
extern "C" uint64_t qsim_subsystem_sweeps_launched(void) { return g_subsystem_sweeps.load(); }

extern "C" int qsim_subsystem_density(qsim_state *s, const int *qubits, int k, double *out_re_im) {
    const char *who = "qsim_subsystem_density";
    if (!s || !out_re_im) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    SubsystemPlan p;
    if (!subsystem_plan(qubits, k, s->n, s->f32, &p))
        return fail(QSIM_ERR_ARG, "%s: 0 to %d distinct qubits inside the register of %d, not more than it has", who, kSubsystemMaxQubits, s->n);
    if (p.path == 2) return qsim_reduced_density(s, qubits, k, out_re_im);
    const size_t entries = (size_t)1 << (2 * k);
    if (qsim_holds_nothing(s)) { // the zero vector: zeros, no sweep
        std::fill(out_re_im, out_re_im + 2 * entries, 0.0);
        return QSIM_OK;
    }
    QSIM_TRY(await_buffer(s));
    HIP_TRY(hipSetDevice(s->device));
    double *d_scratch = nullptr; // per call, before anything is launched
    HIP_TRY(hipMalloc((void **)&d_scratch, p.scratch_bytes));
    const size_t count = p.path ? (size_t)p.upper_blocks * kSubBlockDoubles : 2 * entries;
    std::vector<double> res(count);
    int rc = settle(s);
    if (rc == QSIM_OK) {
        hipError_t e = launch_subsystem(s->stream, s->amps, p, d_scratch);
        if (e == hipSuccess) {
            g_subsystem_sweeps++;
            e = hipMemcpyAsync(res.data(), subsystem_result(p, d_scratch), count * sizeof(double), hipMemcpyDeviceToHost, s->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) rc = fail(QSIM_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    }
    (void)hipFree(d_scratch);
    if (rc != QSIM_OK) return rc;

    std::vector<cplx> rho;
    if (p.path) rho = rho_from_blocks(p, res.data());
    else {
        rho.resize(entries);
        const size_t dim = (size_t)1 << k;
        for (size_t a = 0; a < dim; a++)
            for (size_t b = a; b < dim; b++) { // the upper triangle as computed, the lower its conjugate, the diagonal real
                const cplx v(res[2 * (a * dim + b)], a == b ? 0.0 : res[2 * (a * dim + b) + 1]);
                rho[a * dim + b] = v, rho[b * dim + a] = std::conj(v);
            }
        for (size_t a = 0; a < dim; a++) rho[a * dim + a] = cplx(rho[a * dim + a].real(), 0.0);
    }
    to_callers_order(p, qubits, rho, out_re_im);
    return QSIM_OK;
}

// Undocumented: the time of `instructions` v_mfma_f64_16x16x4_f64 per wave, register operands, in `workgroups` workgroups of four
// waves that each reserve lds_bytes of LDS (so that as many are resident as of the sweep).  tools/subsystem_bench.py's arithmetic floor.
extern "C" int qsim_debug_mfma_f64_probe(long instructions, int workgroups, int lds_bytes, double *ms) {
    const char *who = "qsim_debug_mfma_f64_probe";
    if (!ms) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    float t = 0.0f;
    const hipError_t e = launch_mfma_probe(instructions, workgroups, lds_bytes, &t);
    if (e == hipErrorInvalidValue) return fail(QSIM_ERR_ARG, "%s: at least 16 instructions, 1 to 65536 workgroups, 0 to 160 KiB", who);
    if (e != hipSuccess) return fail(QSIM_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    *ms = t;
    return QSIM_OK;
}
