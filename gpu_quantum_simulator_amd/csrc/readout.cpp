// readout.cpp — everything that looks at a state's amplitudes without changing it, plus qsim_write: amplitudes in and out, the
// norm and the measurement post-path (sampling, block sums and gathers); expectation values of Pauli strings are pauli.cpp's.
// Every entry point opens with settle() or qsim_sync (engine.cpp) and then only reads qsim_state's buffer,
// stream and scratch; nothing here touches the gate queue, the plans or the planning tables.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "engine_state.h"
#include "pauli_sweep.h"

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
    QSIM_TRY(alloc_sweep_scratch(s));
    // The expectation value of the identity string (x = z = 0), as qsim_lanczos_ground takes its start vector's norm: one read-only
    // sweep whose partial sums are added in a fixed order, so equal calls on equal bits return equal bits.  (The sums of k_norm2 met
    // in one atomicAdd, in whatever order the workgroups finished: a lazily held state and its dense copy differed in the last bit.)
    ExpectSweep sw{};
    sw.count = 1;
    const LaunchCfg cfg{s->stream, s->grid_cap};
    QSIM_TRY(launched("norm sweep", launch_expect(cfg, s->amps, s->amps, s->f32, s->n, sw, sweep_partials(s), sweep_result_row(s))));
    return fetch_sweep_results(s, 1, out);
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
