// density.cpp — reduced density matrices of qubit subsets: the plan (the one place that decides the path, the padding and the
// geometry), the entry points, and the way back from the kernel's result to rho in the caller's qubit order.  The
// kernels are density.hip's; density.h has the decomposition they share with this file.  Read-only: the call settles the state,
// reads it once and writes nothing but its own scratch, which is allocated per call before anything is launched.
#include <atomic>
#include <complex>

#include "density.h"
#include "engine_state.h"

using namespace qsim;

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
bool qsim::density_plan(const int *qubits, int k, int n, bool f32, DensityPlan *out) {
    uint64_t mask;
    if (n < 0 || n > 40 || k > kDensityMaxQubits || !qubit_list_mask(qubits, k, n, 0, &mask)) return false;
    DensityPlan p{};
    p.n = n, p.k = k, p.f32 = f32;
    p.units = (1ULL << n) >> (f32 ? 1 : 0);
    if (p.units == 0) p.units = 1; // one fp32 amplitude
    const int kk = k < kDensityMinKernelQubits ? kDensityMinKernelQubits : k;
    // the matrix path: a tile of 16 rows of R and four environments per instruction
    p.path = n >= kDensityMinKernelQubits && n - kk >= 2 ? 1 : 0;
    p.padded_k = p.path ? kk : k;
    p.mask = p.path ? pad_subset(mask, 0, kk, n) : mask;
    p.q0_in = p.mask & 1ULL;
    p.trips_at_cap = 1;
    if (p.path) {
        p.env_units = ctrl_geom(p.mask, 0, f32, n).units;
        const uint64_t per_trip = (uint64_t)kDensityWaves * density_steps_per_trip(density_loads(density_row_units(f32, kk, p.q0_in)));
        p.trips_at_cap = trips_at_cap((p.env_units + 3) >> 2, per_trip, kExpectGrid);
    }
    *out = p;
    return true;
}

extern "C" int qsim_reduced_density_max_qubits(void) { return kDensityMaxQubits; }

extern "C" int qsim_reduced_density_plan(const int *qubits, int k, int num_q, int precision_bits, int *path, int *padded_k, uint64_t *kernel_mask,
                                         uint64_t *units_visited, long *trips_per_workgroup_at_grid_cap) {
    const char *who = "qsim_reduced_density_plan";
    if (!path || !padded_k || !kernel_mask || !units_visited || !trips_per_workgroup_at_grid_cap) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    DensityPlan p;
    if (!density_plan(qubits, k, num_q, precision_bits == 32, &p))
        return fail(QSIM_ERR_ARG, "%s: 0 to %d distinct qubits inside the register, not more than it has", who, kDensityMaxQubits);
    subset_probe_outputs(p, path, padded_k, kernel_mask, units_visited, trips_per_workgroup_at_grid_cap);
    return QSIM_OK;
}

// ---- from the kernel's result to rho ------------------------------------------------------------------------------------------------
using cplx = std::complex<double>;

// rho over the kernel's sorted subset, 2^padded_k square and Hermitian, from a result row of the matrix path: Re rho = G_RR + G_II,
// Im rho = G_IR - G_RI for the upper triangle, the lower one its conjugate.
static std::vector<cplx> rho_from_tiles(const DensityPlan &p, const double *g) {
    const int dim = 1 << p.padded_k, tiles = density_tiles(p.padded_k);
    std::vector<int> at(2 * dim); // row (part, a) of R -> tile * 16 + lane row
    for (int t = 0; t < tiles; t++)
        for (int i = 0; i < 16; i++) {
            int part, a;
            density_row(p, t, i, &part, &a);
            at[part * dim + a] = t * 16 + i;
        }
    auto G = [&](int r, int c) {
        int s = at[r] >> 4, i = at[r] & 15, t = at[c] >> 4, j = at[c] & 15;
        if (s > t) std::swap(s, t), std::swap(i, j); // G is symmetric and only its upper tiles exist
        return g[density_element(tiles, s, t, i, j)];
    };
    std::vector<cplx> rho((size_t)dim * dim);
    for (int a = 0; a < dim; a++)
        for (int b = a; b < dim; b++) {
            const cplx v(G(a, b) + G(dim + a, dim + b), G(dim + a, b) - G(a, dim + b));
            rho[(size_t)a * dim + b] = v;
            rho[(size_t)b * dim + a] = std::conj(v);
        }
    return rho;
}

// out = rho in the caller's qubit order: bit j of an index is qubit qubits[j]; the kernel's qubits that are not the caller's (the
// padding) are traced out, their values added in ascending order.  Hermitian bit for bit: the lower triangle is the upper one's
// conjugate and the diagonal is real.
static void to_callers_order(const DensityPlan &p, const int *qubits, const std::vector<cplx> &rho, double *out) {
    const int kdim = 1 << p.padded_k, dim = 1 << p.k;
    const SubsetOrder order{p.mask, qubits, p.k};
    const uint32_t own = order.own();
    std::vector<uint32_t> base(dim), pad;
    for (int c = 0; c < dim; c++) base[c] = order.to_subset(c);
    for (uint32_t v = 0; v < (uint32_t)kdim; v++)
        if (!(v & own)) pad.push_back(v);
    for (int a = 0; a < dim; a++)
        for (int b = a; b < dim; b++) {
            cplx v = 0.0;
            for (uint32_t t : pad) v += rho[(size_t)(base[a] | t) * kdim + (base[b] | t)];
            if (a == b) v = cplx(v.real(), 0.0);
            out[2 * ((size_t)a * dim + b)] = v.real(), out[2 * ((size_t)a * dim + b) + 1] = v.imag();
            out[2 * ((size_t)b * dim + a)] = v.real(), out[2 * ((size_t)b * dim + a) + 1] = -v.imag();
        }
    for (int a = 0; a < dim; a++) out[2 * ((size_t)a * dim + a) + 1] = 0.0; // not -0
}

// ---- the call ---------------------------------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_density_sweeps{0};
extern "C" uint64_t qsim_density_sweeps_launched(void) { return g_density_sweeps.load(); }

extern "C" int qsim_reduced_density(qsim_state *s, const int *qubits, int k, double *out_re_im) {
    const char *who = "qsim_reduced_density";
    if (!s || !out_re_im) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    DensityPlan p;
    if (!density_plan(qubits, k, s->n, s->f32, &p))
        return fail(QSIM_ERR_ARG, "%s: 0 to %d distinct qubits inside the register of %d, not more than it has", who, kDensityMaxQubits, s->n);
    const size_t entries = (size_t)1 << (2 * k);
    if (qsim_holds_nothing(s)) { // the zero vector: zeros, no sweep
        std::fill(out_re_im, out_re_im + 2 * entries, 0.0);
        return QSIM_OK;
    }
    QSIM_TRY(await_buffer(s));
    HIP_TRY(hipSetDevice(s->device));
    double *d_scratch = nullptr; // up to 1025 rows of 9216 doubles, far above kSweepScratchDoubles: per call, before anything is launched
    HIP_TRY(hipMalloc((void **)&d_scratch, density_scratch_doubles(p) * sizeof(double)));
    const size_t count = p.path ? (size_t)density_row_doubles(p.padded_k) : 2 * entries;
    std::vector<double> res(count);
    int rc = settle(s);
    if (rc == QSIM_OK) {
        const LaunchCfg cfg{s->stream, s->grid_cap};
        hipError_t e = launch_density(cfg, s->amps, p, d_scratch);
        if (e == hipSuccess) {
            g_density_sweeps++;
            e = hipMemcpyAsync(res.data(), density_result(p, d_scratch), count * sizeof(double), hipMemcpyDeviceToHost, s->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) rc = fail(QSIM_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    }
    (void)hipFree(d_scratch);
    if (rc != QSIM_OK) return rc;

    std::vector<cplx> rho;
    if (p.path) rho = rho_from_tiles(p, res.data());
    else {
        rho.resize(entries);
        for (size_t el = 0; el < entries; el++) rho[el] = cplx(res[2 * el], res[2 * el + 1]);
    }
    to_callers_order(p, qubits, rho, out_re_im);
    return QSIM_OK;
}
