// readout.cpp — everything that looks at a state without changing it, plus qsim_write: amplitudes in and out, the norm,
// expectation values of Pauli strings (the host side of expect.hip's sweeps) and the measurement post-path (sampling, block
// sums and gathers).  Every entry point opens with settle() or qsim_sync (engine.cpp) and then only reads qsim_state's buffer,
// stream and scratch; nothing here touches the gate queue, the plans or the planning tables.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "engine_state.h"

using namespace qsim;

// ---- amplitudes ----------------------------------------------------------------------------------------
// `out` holds m doubles' worth of room and m floats in its second half: widen them front to back (element i is read
// from byte 4m + 4i before byte 8i is written, and no later element starts below 8i + 8).
static void widen_in_place(double *out, uint64_t m) {
    const char *src = reinterpret_cast<const char *>(out) + 4 * m;
    for (uint64_t i = 0; i < m; i++) {
        float f;
        memcpy(&f, src + 4 * i, 4);
        out[i] = (double)f;
    }
}

// `count` amplitudes from `first` on as (re, im) doubles, whatever the state's precision; blocks until they are there.
static int read_amps(qsim_state *s, uint64_t first, uint64_t count, double *out) {
    if (!s->f32) {
        HIP_TRY(hipMemcpy(out, (const char *)s->amps + first * 16, count * 16, hipMemcpyDeviceToHost));
        return QSIM_OK;
    }
    // fp32 state: the API stays double; copy into the second half of the output and widen in place, front to back
    char *tmp = reinterpret_cast<char *>(out) + 8 * count;
    HIP_TRY(hipMemcpy(tmp, (const char *)s->amps + first * 8, count * 8, hipMemcpyDeviceToHost));
    widen_in_place(out, 2 * count);
    return QSIM_OK;
}

extern "C" int qsim_read(qsim_state *s, uint64_t first, uint64_t count, double *out) {
    if (!s || !out) return fail(QSIM_ERR_ARG, "NULL argument");
    const uint64_t N = 1ULL << s->n;
    if (first > N || count > N - first) return fail(QSIM_ERR_ARG, "read range outside the state");
    QSIM_TRY(qsim_sync(s));
    HIP_TRY(hipSetDevice(s->device));
    return count ? read_amps(s, first, count, out) : QSIM_OK;
}

extern "C" int qsim_write(qsim_state *s, uint64_t first, uint64_t count, const double *in) {
    if (!s || !in) return fail(QSIM_ERR_ARG, "NULL argument");
    const uint64_t N = 1ULL << s->n;
    if (first > N || count > N - first) return fail(QSIM_ERR_ARG, "write range outside the state");
    QSIM_TRY(qsim_sync(s));
    HIP_TRY(hipSetDevice(s->device));
    if (!count) return QSIM_OK;
    if (!s->f32) {
        HIP_TRY(hipMemcpy((char *)s->amps + first * 16, in, count * 16, hipMemcpyHostToDevice));
        return QSIM_OK;
    }
    std::vector<float> tmp(2 * count);
    for (uint64_t i = 0; i < 2 * count; i++) tmp[i] = (float)in[i];
    HIP_TRY(hipMemcpy((char *)s->amps + first * 8, tmp.data(), count * 8, hipMemcpyHostToDevice));
    return QSIM_OK;
}

extern "C" int qsim_norm2(qsim_state *s, double *out) {
    if (!s || !out) return fail(QSIM_ERR_ARG, "NULL argument");
    QSIM_TRY(settle(s));
    HIP_TRY(hipMemsetAsync(s->d_scalar, 0, 8, s->stream));
    LaunchCfg cfg{s->stream, s->grid_cap};
    HIP_TRY(launch_norm2(cfg, s->amps, s->f32, s->n, s->d_scalar));
    HIP_TRY(hipMemcpyAsync(out, s->d_scalar, 8, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return QSIM_OK;
}

// ---- expectation values of Pauli strings (expect.hip; DESIGN "Expectation values") ----------------------------------------------
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
    constexpr int kBatch = 128; // sweeps whose results travel in one copy
    if (!s->d_expect) HIP_TRY(hipMalloc((void **)&s->d_expect, (kExpectPartialDoubles + (size_t)kBatch * kMaxTermsPerSweep) * sizeof(double)));
    double *d_results = s->d_expect + kExpectPartialDoubles;
    const PauliSweeps plan = pauli_sweeps(X, mmask, num);
    std::vector<double> host((size_t)kBatch * kMaxTermsPerSweep);
    LaunchCfg cfg{s->stream, s->grid_cap};
    for (size_t first = 0; first < plan.sweeps.size(); first += kBatch) {
        const size_t last = std::min(plan.sweeps.size(), first + (size_t)kBatch);
        for (size_t w = first; w < last; w++) {
            ExpectSweep sw{};
            sw.x = X[plan.order[(size_t)plan.sweeps[w].first]] & mmask;
            sw.full = x_rank != 0;
            sw.count = plan.sweeps[w].second;
            for (int k = 0; k < sw.count; k++) {
                const long t = plan.order[(size_t)(plan.sweeps[w].first + k)];
                sw.z[k] = Z[t] & mmask;
                if (__builtin_popcountll(X[t] & Z[t]) & 1) sw.im_mask |= 1u << k;
            }
            HIP_TRY(launch_expect(cfg, s->amps, partner ? partner : s->amps, s->f32, m, sw, s->d_expect, d_results + (w - first) * kMaxTermsPerSweep));
        }
        HIP_TRY(hipMemcpyAsync(host.data(), d_results, (last - first) * kMaxTermsPerSweep * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        for (size_t w = first; w < last; w++)
            for (int k = 0; k < plan.sweeps[w].second; k++) {
                const long t = plan.order[(size_t)(plan.sweeps[w].first + k)];
                const int ny = __builtin_popcountll(X[t] & Z[t]);
                // i^ny (c + (-1)^ny conj c): 2 Re c, -2 Im c, -2 Re c, 2 Im c for ny = 0, 1, 2, 3 mod 4; x == 0: the plain signed norm
                double f = X[t] == 0 ? 1.0 : ((ny & 3) == 0 || (ny & 3) == 3 ? 2.0 : -2.0);
                if (__builtin_popcountll(rank & (Z[t] >> m)) & 1) f = -f; // Z on rank qubits: a sign per shard
                out[t] = f * host[(w - first) * kMaxTermsPerSweep + (size_t)k];
            }
    }
    return QSIM_OK;
}

extern "C" int qsim_expect_paulis(qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, double *out) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    if (num_terms < 0) return fail(QSIM_ERR_ARG, "qsim_expect_paulis: negative term count");
    if (num_terms > 0 && (!x_masks || !z_masks || !out)) return fail(QSIM_ERR_ARG, "qsim_expect_paulis: NULL argument");
    const uint64_t nmask = index_mask(s->n);
    for (long t = 0; t < num_terms; t++)
        if ((x_masks[t] | z_masks[t]) & ~nmask)
            return fail(QSIM_ERR_ARG, "qsim_expect_paulis: term %ld names a qubit outside the %d-qubit register", t, s->n);
    return expect_paulis_shard(s, nullptr, 0, x_masks, z_masks, num_terms, out);
}

// ---- measurement post-path ----------------------------------------------------------------------------------
// Runs `launch` on a temporary device buffer of `bytes`, copies the buffer to `host` and waits for it.
template <class Launch>
static int fetch_from_device(qsim_state *s, const char *who, size_t bytes, void *host, Launch launch) {
    void *d_buf = nullptr;
    HIP_TRY(hipMalloc(&d_buf, bytes));
    hipError_t e = launch(d_buf);
    if (e == hipSuccess) e = hipMemcpyAsync(host, d_buf, bytes, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    (void)hipFree(d_buf);
    if (e != hipSuccess) return fail(QSIM_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return QSIM_OK;
}

extern "C" double qsim_draw_randn(void) { // measurement, quantum_simulator.c:271-276
    double randn = 0.0, coeff = 1.0 / RAND_MAX;
    for (int i = 0; i < 10; i++) {
        randn += rand() * coeff;
        coeff *= 1.0 / RAND_MAX;
    }
    return randn;
}

extern "C" void qsim_putb(long long n, int len, char *buf) { // putb, quantum_simulator.c:285-293
    if (!buf || len < 0) return;
    for (int k = 0; k < len; k++) buf[k] = ((n >> (len - 1 - k)) & 1) ? '1' : '0';
    buf[len] = 0;
}

extern "C" int qsim_sample(qsim_state *s, const double *randoms, long shots, uint64_t *out) {
    if (!s || (shots > 0 && (!randoms || !out))) return fail(QSIM_ERR_ARG, "NULL argument");
    QSIM_TRY(settle(s));
    constexpr int kBlockBits = 12;
    const uint64_t N = 1ULL << s->n;
    const int bb = s->n < kBlockBits ? s->n : kBlockBits;
    const uint64_t nblocks = N >> bb, bsize = 1ULL << bb;
    const LaunchCfg cfg{s->stream, s->grid_cap};
    std::vector<double> prefix(nblocks);
    QSIM_TRY(fetch_from_device(s, "qsim_sample", nblocks * sizeof(double), prefix.data(), [&](void *d) { return launch_block_prob(cfg, s->amps, s->f32, s->n, bb, (double *)d); }));
    double acc = 0.0;
    for (uint64_t b = 0; b < nblocks; b++) { acc += prefix[b]; prefix[b] = acc; } // cumulative at the END of block b

    std::vector<double> blk(2 * bsize);
    uint64_t cached = ~0ULL;
    for (long k = 0; k < shots; k++) {
        const double r = randoms[k];
        // first block whose end value is non-zero and >= r (quantum_simulator.c:279: skip while == 0 or < r)
        uint64_t lo = 0, hi = nblocks;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (prefix[mid] == 0.0 || prefix[mid] < r) lo = mid + 1;
            else hi = mid;
        }
        uint64_t idx = N - 1;
        bool found = false;
        for (uint64_t b = lo; b < nblocks && !found; b++) { // normally one block; rounding can push it to the next
            if (b != cached) {
                QSIM_TRY(read_amps(s, b * bsize, bsize, blk.data()));
                cached = b;
            }
            double c = b ? prefix[b - 1] : 0.0;
            for (uint64_t i = 0; i < bsize; i++) {
                c += blk[2 * i] * blk[2 * i] + blk[2 * i + 1] * blk[2 * i + 1];
                if (!(c == 0.0 || c < r)) { idx = b * bsize + i; found = true; break; }
            }
        }
        out[k] = idx;
    }
    return QSIM_OK;
}

// Block sums and block contents for index sets that are bit-deposits rather than ranges (what a permuted qubit map of a
// sharded state needs for the measurement post-path; see k_block_prob_masked).
extern "C" int qsim_block_prob_masked(qsim_state *s, uint64_t hi_mask, uint64_t lo_mask, double *out) {
    if (!s || !out) return fail(QSIM_ERR_ARG, "NULL argument");
    const uint64_t all = index_mask(s->n);
    if ((hi_mask & lo_mask) || ((hi_mask | lo_mask) & ~all)) return fail(QSIM_ERR_ARG, "masks must be disjoint and inside the state");
    QSIM_TRY(settle(s));
    const uint64_t nblocks = 1ULL << __builtin_popcountll(hi_mask);
    const LaunchCfg cfg{s->stream, s->grid_cap};
    return fetch_from_device(s, "qsim_block_prob_masked", nblocks * sizeof(double), out, [&](void *d) { return launch_block_prob_masked(cfg, s->amps, s->f32, hi_mask, lo_mask, (double *)d); });
}

extern "C" int qsim_gather_masked(qsim_state *s, uint64_t base, uint64_t lo_mask, double *out) {
    if (!s || !out) return fail(QSIM_ERR_ARG, "NULL argument");
    const uint64_t all = index_mask(s->n);
    if ((base & lo_mask) || ((base | lo_mask) & ~all)) return fail(QSIM_ERR_ARG, "base and mask must be disjoint and inside the state");
    const uint64_t count = 1ULL << __builtin_popcountll(lo_mask);
    if (count > (1ULL << 24)) return fail(QSIM_ERR_ARG, "gather of %llu amplitudes is not a block", (unsigned long long)count);
    QSIM_TRY(settle(s));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    void *host = s->f32 ? reinterpret_cast<char *>(out) + 8 * count : (char *)out; // fp32: into the second half, widened in place below
    QSIM_TRY(fetch_from_device(s, "qsim_gather_masked", count * s->amp_bytes(), host, [&](void *d) { return launch_gather_masked(cfg, s->amps, s->f32, base, lo_mask, d); }));
    if (s->f32) widen_in_place(out, 2 * count);
    return QSIM_OK;
}
