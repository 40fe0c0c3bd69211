// lanczos.cpp — the lowest eigenvalue of a Pauli-sum Hamiltonian, and optionally its eigenvector, by the Lanczos recurrence on the
// device.  A step is three things that exist elsewhere: w = H v (pauli_sum_sweeps, pauli.cpp), alpha = Re <v|w>
// (launch_expect over two buffers, expect.hip) and w <- w - alpha v - beta u with |w|^2 from the same sweep (launch_combine,
// combine.hip).  This file has the recurrence, the small tridiagonal eigenproblem on the host and the buffer bookkeeping.
//
// Recurrence, in this order:  v_0 = state / |state|;  for j = 0, 1, ...:  w = H v_j;  alpha_j = Re <v_j|w>;
// w <- w - alpha_j v_j - beta_(j-1) v_(j-1);  beta_j = |w|;  v_(j+1) = w / beta_j.  No reorthogonalisation: the lowest Ritz value
// converges without it (ghost copies of converged Ritz values appear, they do not move the extreme one), which is also why no
// interior eigenvalue is offered.
// No normalising sweep: the buffers hold the UNNORMALISED vectors w, whose norms nu_j (nu_0 = |state|, nu_(j+1) = beta_j) the host
// knows; 1/nu_j is folded into the coefficients of H for the next application and into the coefficients of the update.
// Host synchronisation: two small ones per step, for alpha and for beta — each decides the coefficients of the next launch.
// Memory: the state and three work buffers, whatever the number of steps.  The first pass only READS the state's buffer.  With
// want_vector a second pass re-runs the recurrence with the recorded alpha and beta (no reduction is waited for) and accumulates
// y = sum_j t_j v_j in the state's own buffer, v_0 having been copied aside.
#include <algorithm>
#include <cmath>
#include <vector>

#include "engine_state.h"
#include "pauli_sweep.h"

using namespace qsim;

// ---- the tridiagonal eigenproblem (host only) ----------------------------------------------------------------------------------
// eigenvalues of T below x: the negative pivots of the LDL^T of T - x (Sturm count); a zero pivot is nudged off zero
static int count_below(const double *al, const double *be, int m, double x, double tiny) {
    int count = 0;
    double d = 1.0;
    for (int i = 0; i < m; i++) {
        d = (al[i] - x) - (i > 0 ? be[i - 1] * be[i - 1] / d : 0.0);
        if (std::fabs(d) < tiny) d = -tiny;
        if (d < 0.0) count++;
    }
    return count;
}

extern "C" int qsim_tridiag_lowest(const double *alphas, const double *betas, int m, double *theta, double *vec) {
    if (m < 1 || !alphas || !theta || (m > 1 && !betas)) return fail(QSIM_ERR_ARG, "qsim_tridiag_lowest: bad argument");
    double norm = 0.0, bmax = 0.0;
    for (int i = 0; i < m; i++) {
        if (!std::isfinite(alphas[i]) || (i + 1 < m && !std::isfinite(betas[i]))) return fail(QSIM_ERR_ARG, "qsim_tridiag_lowest: a non-finite entry");
        norm = std::max(norm, std::fabs(alphas[i]));
        if (i + 1 < m) bmax = std::max(bmax, std::fabs(betas[i]));
    }
    norm += 2.0 * bmax; // Gershgorin: every eigenvalue lies in [-norm, norm]
    if (m == 1 || norm == 0.0) {
        *theta = m == 1 ? alphas[0] : 0.0;
        if (vec) {
            std::fill(vec, vec + m, 0.0);
            vec[0] = 1.0;
        }
        return QSIM_OK;
    }
    // bisection for the lowest eigenvalue, until the interval no longer splits
    const double tiny = norm * 0x1p-60;
    double lo = -norm * (1.0 + 0x1p-40), hi = norm * (1.0 + 0x1p-40);
    for (int it = 0; it < 200; it++) {
        const double mid = lo + 0.5 * (hi - lo);
        if (mid <= lo || mid >= hi) break;
        if (count_below(alphas, betas, m, mid, tiny) >= 1) hi = mid;
        else lo = mid;
    }
    const double th = lo + 0.5 * (hi - lo);
    *theta = th;
    if (!vec) return QSIM_OK;
    // inverse iteration: (T - theta) x = b by Gaussian elimination with partial pivoting (an upper triangle of three diagonals), a
    // pivot at rounding level replaced by that level; a fixed start vector, so equal inputs give equal bits
    std::vector<double> u0(m), u1(m), u2(m), l(m), x(m);
    std::vector<char> swapped(m);
    const double eps = norm * 0x1p-52;
    {
        double d = alphas[0] - th, e = betas[0]; // the current row: (d, e, 0) at columns i, i + 1, i + 2
        for (int i = 0; i + 1 < m; i++) {
            const double sub = betas[i], nd = alphas[i + 1] - th, ne = i + 2 < m ? betas[i + 1] : 0.0; // next row: (sub, nd, ne)
            if (std::fabs(sub) > std::fabs(d)) { // swap the rows
                swapped[i] = 1;
                l[i] = d / sub;
                u0[i] = sub, u1[i] = nd, u2[i] = ne;
                d = e - l[i] * nd;
                e = -l[i] * ne;
            } else {
                swapped[i] = 0;
                if (std::fabs(d) < eps) d = d < 0.0 ? -eps : eps;
                l[i] = sub / d;
                u0[i] = d, u1[i] = e, u2[i] = 0.0;
                d = nd - l[i] * e;
                e = ne;
            }
        }
        if (std::fabs(d) < eps) d = d < 0.0 ? -eps : eps;
        u0[m - 1] = d, u1[m - 1] = 0.0, u2[m - 1] = 0.0;
    }
    uint64_t seed = 0x9E3779B97F4A7C15ULL;
    for (int i = 0; i < m; i++) {
        seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
        x[i] = 0.5 + (double)(seed >> 11) * 0x1p-53;
    }
    for (int it = 0; it < 5; it++) {
        for (int i = 0; i + 1 < m; i++) { // forward: the row operations on b
            if (swapped[i]) std::swap(x[i], x[i + 1]);
            x[i + 1] -= l[i] * x[i];
        }
        for (int i = m - 1; i >= 0; i--) { // back substitution
            double v = x[i];
            if (i + 1 < m) v -= u1[i] * x[i + 1];
            if (i + 2 < m) v -= u2[i] * x[i + 2];
            x[i] = v / u0[i];
        }
        double big = 0.0;
        for (int i = 0; i < m; i++) big = std::max(big, std::fabs(x[i]));
        if (!(big > 0.0) || !std::isfinite(big)) return fail(QSIM_ERR_DEVICE, "qsim_tridiag_lowest: inverse iteration broke down");
        double s2 = 0.0;
        for (int i = 0; i < m; i++) {
            x[i] /= big;
            s2 += x[i] * x[i];
        }
        const double inv = 1.0 / std::sqrt(s2);
        for (int i = 0; i < m; i++) x[i] *= inv;
    }
    // sign: the largest component positive
    int arg = 0;
    for (int i = 1; i < m; i++)
        if (std::fabs(x[i]) > std::fabs(x[arg])) arg = i;
    const double sign = x[arg] < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < m; i++) vec[i] = sign * x[i];
    return QSIM_OK;
}

// ---- the plan (host only) ----------------------------------------------------------------------------------------------------------
static int check_run(const char *who, int max_steps, double tol) {
    if (max_steps < 1) return fail(QSIM_ERR_ARG, "%s: max_steps is %d", who, max_steps);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(QSIM_ERR_ARG, "%s: tol is negative or not finite", who);
    return QSIM_OK;
}

extern "C" int qsim_lanczos_plan(const uint64_t *ham_x, long num_ham, int max_steps, int want_vector, long *sum_sweeps_per_step,
                                 long *other_sweeps_per_step, double *volumes_per_step) {
    (void)want_vector; // the second pass repeats the steps; what ONE step of the first pass costs does not depend on it
    if (!sum_sweeps_per_step || !other_sweeps_per_step || !volumes_per_step) return fail(QSIM_ERR_ARG, "qsim_lanczos_plan: NULL argument");
    QSIM_TRY(check_run("qsim_lanczos_plan", max_steps, 0.0));
    QSIM_TRY(qsim_pauli_sweeps(ham_x, num_ham, sum_sweeps_per_step)); // the grouping pauli_sum_sweeps launches by
    *other_sweeps_per_step = 2;                                         // alpha, and the update
    // H: the first sweep reads the source and writes (2 volumes), every other one reads the destination as well (3); H = 0: one fill
    const double h = *sum_sweeps_per_step > 0 ? 3.0 * (double)*sum_sweeps_per_step - 1.0 : 1.0;
    *volumes_per_step = h + 2.0 /* alpha reads v and w */ + 4.0 /* the update reads w, v, u and writes w */;
    return QSIM_OK;
}

// ---- the solver ----------------------------------------------------------------------------------------------------------------------
namespace {

struct WorkBuffers { // three buffers of the state's size: the idle spare buffer and d_adjoint where they exist, the rest allocated here
    void *buf[3] = {nullptr, nullptr, nullptr};
    void *mine[3] = {nullptr, nullptr, nullptr};
    int acquire(qsim_state *s) {
        int have = 0;
        if (s->spare && s->spare != s->amps) buf[have++] = s->spare;
        if (s->d_adjoint) buf[have++] = s->d_adjoint;
        for (; have < 3; have++) {
            HIP_TRY(hipMalloc(&mine[have], s->amp_bytes() << s->n));
            buf[have] = mine[have];
        }
        return QSIM_OK;
    }
    void *other_than(const void *a, const void *b) const { // a work buffer that holds neither of two live vectors
        for (void *p : buf)
            if (p != a && p != b) return p;
        return nullptr;
    }
    ~WorkBuffers() {
        for (void *p : mine)
            if (p) (void)hipFree(p);
    }
};

struct Run {
    qsim_state *s;
    const uint64_t *X, *Z;
    const double *C;
    long num;
    void *home;                 // the state's own buffer
    std::vector<double> scaled; // coeffs / nu
    LaunchCfg cfg;

    // dst = H src / nu: pauli_sum_sweeps reads s->amps, which stands in for the source while it runs
    int apply_h(void *src, double nu, void *dst) {
        for (long t = 0; t < num; t++) scaled[(size_t)t] = C[t] / nu;
        s->amps = src;
        const int rc = pauli_sum_sweeps(s, X, Z, scaled.data(), num, dst);
        s->amps = home;
        return rc;
    }
    int combine(void *dst, double d, const void *p, double a, const void *q, double b) {
        const double dd[2] = {d, 0.0}, aa[2] = {a, 0.0}, bb[2] = {b, 0.0};
        return launched("combine", launch_combine(cfg, dst, dd, p, aa, q, bb, s->f32, s->n, sweep_partials(s), sweep_result_row(s)));
    }
    int result(double *out) { return fetch_sweep_results(s, 1, out); }
};

} // namespace

extern "C" int qsim_lanczos_ground(qsim_state *s, const uint64_t *ham_x, const uint64_t *ham_z, const double *coeffs, long num_ham, int max_steps,
                                   double tol, int want_vector, double *energy, double *residual, int *steps, double *alphas, double *betas) {
    const char *who = "qsim_lanczos_ground";
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    QSIM_TRY(check_pauli_terms(fail, who, s->n, ham_x, ham_z, coeffs, coeffs, num_ham, "coefficient"));
    QSIM_TRY(check_run(who, max_steps, tol));
    if (qsim_holds_nothing(s)) return fail(QSIM_ERR_ARG, "%s: the state holds nothing", who);
    QSIM_TRY(await_buffer(s));
    HIP_TRY(hipSetDevice(s->device));
    // everything that can fail for want of memory comes before the state is touched
    WorkBuffers work;
    QSIM_TRY(work.acquire(s));
    QSIM_TRY(alloc_sweep_scratch(s));
    QSIM_TRY(settle(s));

    Run run{s, ham_x, ham_z, coeffs, num_ham, s->amps, std::vector<double>((size_t)num_ham), LaunchCfg{s->stream, s->grid_cap}};
    double csum = 0.0;
    for (long t = 0; t < num_ham; t++) csum += std::fabs(coeffs[t]);
    const double floor_beta = 64.0 * (s->f32 ? 0x1p-24 : 0x1p-53) * csum; // the rounding level of w: the Krylov space is exhausted

    // nu_0 = |state|: the squared norm as one unpaired sweep
    double nu0;
    {
        ExpectSweep sw{};
        sw.count = 1;
        QSIM_TRY(launched("norm", launch_expect(run.cfg, s->amps, s->amps, s->f32, s->n, sw, sweep_partials(s), sweep_result_row(s))));
        QSIM_TRY(run.result(&nu0));
        if (!(nu0 > 0.0) || !std::isfinite(nu0)) return fail(QSIM_ERR_ARG, "%s: the state has norm zero (or is not finite)", who);
        nu0 = std::sqrt(nu0);
    }

    // ---- first pass: alpha, beta and the Ritz value; the state's buffer is only read
    std::vector<double> al, be, nu{nu0}, t;
    double theta = 0.0, estimate = 0.0;
    void *cur = s->amps, *prev = nullptr; // v_j and v_(j-1), unnormalised
    for (int j = 0; j < max_steps; j++) {
        void *w = work.other_than(cur, prev); // never the state's own buffer
        QSIM_TRY(run.apply_h(cur, nu[(size_t)j], w));
        ExpectSweep sw{};
        sw.full = true; // x == 0 over two buffers
        sw.count = 1;
        double a_raw;
        QSIM_TRY(launched("expectation", launch_expect(run.cfg, cur, w, s->f32, s->n, sw, sweep_partials(s), sweep_result_row(s))));
        QSIM_TRY(run.result(&a_raw));
        const double alpha = a_raw / nu[(size_t)j];
        double w2;
        QSIM_TRY(run.combine(w, 1.0, cur, -alpha / nu[(size_t)j], prev, j > 0 ? -be[(size_t)j - 1] / nu[(size_t)j - 1] : 0.0));
        QSIM_TRY(run.result(&w2));
        const double beta = std::sqrt(w2);
        if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(QSIM_ERR_DEVICE, "%s: step %d left a non-finite alpha or beta", who, j);
        al.push_back(alpha);
        be.push_back(beta);
        nu.push_back(beta);
        t.assign((size_t)j + 1, 0.0);
        QSIM_TRY(qsim_tridiag_lowest(al.data(), be.data(), j + 1, &theta, t.data()));
        estimate = beta * std::fabs(t[(size_t)j]);
        if (estimate <= tol || beta <= floor_beta) break;
        prev = cur; // v_(j+1) = w
        cur = w;
    }
    const int m = (int)al.size();
    if (steps) *steps = m;
    if (energy) *energy = theta;
    if (alphas) std::copy(al.begin(), al.end(), alphas);
    if (betas) std::copy(be.begin(), be.end(), betas);
    if (!want_vector) {
        if (residual) *residual = estimate;
        return QSIM_OK;
    }

    // ---- second pass: y = sum_j t_j v_j in the state's own buffer, v_0 copied aside; the recorded alpha and beta, nothing waited for
    void *y = run.home;
    HIP_TRY(hipMemcpyAsync(work.buf[0], y, s->amp_bytes() << s->n, hipMemcpyDeviceToDevice, s->stream));
    QSIM_TRY(run.combine(y, 0.0, work.buf[0], t[0] / nu[0], nullptr, 0.0));
    cur = work.buf[0], prev = nullptr;
    for (int j = 0; j + 1 < m; j++) {
        void *w = work.other_than(cur, prev);
        QSIM_TRY(run.apply_h(cur, nu[(size_t)j], w));
        QSIM_TRY(run.combine(w, 1.0, cur, -al[(size_t)j] / nu[(size_t)j], prev, j > 0 ? -be[(size_t)j - 1] / nu[(size_t)j - 1] : 0.0));
        QSIM_TRY(run.combine(y, 1.0, w, t[(size_t)j + 1] / nu[(size_t)j + 1], nullptr, 0.0));
        prev = cur;
        cur = w;
    }
    double y2;
    QSIM_TRY(run.result(&y2)); // of the last combine: |y|^2
    if (!(y2 > 0.0) || !std::isfinite(y2)) return fail(QSIM_ERR_DEVICE, "%s: the Ritz vector has norm zero (or is not finite)", who);
    const double ny = std::sqrt(y2);
    // the residual, measured: r = H y / |y| - theta y / |y|
    void *r = work.buf[0], *tmp = work.buf[1];
    double r2;
    QSIM_TRY(run.apply_h(y, ny, r));
    QSIM_TRY(run.combine(r, 1.0, y, -theta / ny, nullptr, 0.0));
    QSIM_TRY(run.result(&r2));
    if (residual) *residual = std::sqrt(r2);
    // the state ends as y / |y|: scaled aside (p != dst is the kernel's rule), then copied home — once per call
    QSIM_TRY(run.combine(tmp, 0.0, y, 1.0 / ny, nullptr, 0.0));
    HIP_TRY(hipMemcpyAsync(y, tmp, s->amp_bytes() << s->n, hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // the work buffers go away with this call
    return QSIM_OK;
}
