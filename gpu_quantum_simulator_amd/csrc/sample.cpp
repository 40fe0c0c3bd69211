// sample.cpp — the host side of sample.hip: qsim_sample_geometry (host only), qsim_sample_shots, which draws basis states of one
// state on the device (sample.h has the pyramid), and qsim_sample_stage_times, what the measurement tool times its two
// preparing stages with.  Like readout.cpp's calls it opens with settle() and then only reads the
// state's buffer and stream.  What a call needs on the device — the pyramid's two arrays, the draws and the results — is ONE allocation
// made and freed by the call, as fetch_from_device does it: 0.2 % of the state plus 16 bytes per draw, nothing kept with the state.
#include <cmath>

#include "engine_state.h"
#include "sample.h"

using namespace qsim;

extern "C" int qsim_sample_geometry(int n, int *chunk_bits, int *group_bits, uint64_t *scratch_bytes) {
    const char *who = "qsim_sample_geometry";
    if (!chunk_bits || !group_bits || !scratch_bytes) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    if (n < 0 || n > 40) return fail(QSIM_ERR_ARG, "%s: 0 to 40 qubits, not %d", who, n);
    const SampleGeom g = sample_geom(n);
    *chunk_bits = g.chunk_bits;
    *group_bits = g.chunk_bits + g.group_chunk_bits;
    *scratch_bytes = sample_scratch_bytes(g);
    return QSIM_OK;
}

// What tools/sample_bench.py times the two preparing stages with: device events around each, on a pyramid of the call's own.
extern "C" int qsim_sample_stage_times(qsim_state *s, double *chunk_sums_ms, double *prefix_ms) {
    const char *who = "qsim_sample_stage_times";
    if (!s || !chunk_sums_ms || !prefix_ms) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(settle(s));
    const SampleGeom g = sample_geom(s->n);
    double *d_w = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    HIP_TRY(hipMalloc((void **)&d_w, (size_t)sample_scratch_bytes(g)));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3 && e == hipSuccess; k++) e = hipEventCreate(&ev[k]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], s->stream);
    if (e == hipSuccess) e = launch_sample_chunk_sums(cfg, s->amps, s->f32, s->n, d_w);
    if (e == hipSuccess) e = hipEventRecord(ev[1], s->stream);
    if (e == hipSuccess) e = launch_sample_prefix(cfg, s->n, d_w, d_w + g.chunks);
    if (e == hipSuccess) e = hipEventRecord(ev[2], s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    float a = 0.0f, b = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&a, ev[0], ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&b, ev[1], ev[2]);
    for (hipEvent_t v : ev)
        if (v) (void)hipEventDestroy(v);
    (void)hipFree(d_w);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? QSIM_ERR_ALLOC : QSIM_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    *chunk_sums_ms = a;
    *prefix_ms = b;
    return QSIM_OK;
}

// The body of qsim_sample_shots, for measure.cpp's qsim_measure too (one sampler): `who` names the caller in messages,
// *total (when asked for, and whenever the pyramid was built) is T[last], the sum the draws are scaled by.
int qsim::sample_outcomes(qsim_state *s, const char *who, const double *draws, long shots, const int *qubits, int num_qubits, uint64_t *out, double *total_out) {
    if (!s || shots < 0 || (shots > 0 && (!draws || !out)) || (num_qubits > 0 && !qubits)) return fail(QSIM_ERR_ARG, "%s: NULL argument or a negative count", who);
    if (num_qubits < 0 || num_qubits > kSampleMaxQubits) return fail(QSIM_ERR_ARG, "%s: 0 to %d qubits, not %d", who, kSampleMaxQubits, num_qubits);
    SampleQubits qs{};
    uint64_t seen = 0;
    for (int j = 0; j < num_qubits; j++) {
        const int q = qubits[j];
        if (q < 0 || q >= s->n || ((seen >> q) & 1ULL)) return fail(QSIM_ERR_ARG, "%s: qubit %d (entry %d) is outside the register of %d or repeated", who, q, j, s->n);
        seen |= 1ULL << q;
        qs.q[j] = (uint8_t)q;
    }
    qs.count = num_qubits;
    for (long k = 0; k < shots; k++)
        if (!(draws[k] >= 0.0 && draws[k] <= 1.0)) return fail(QSIM_ERR_ARG, "%s: draw %ld is %g, not a number in [0, 1]", who, k, draws[k]);
    if (shots == 0) return QSIM_OK;
    QSIM_TRY(settle(s));

    const SampleGeom g = sample_geom(s->n);
    const size_t pyramid = (size_t)sample_scratch_bytes(g), list = (size_t)shots * 8;
    char *d_buf = nullptr;
    HIP_TRY(hipMalloc((void **)&d_buf, pyramid + 2 * list));
    double *d_w = (double *)d_buf, *d_t = d_w + g.chunks, *d_draws = (double *)(d_buf + pyramid);
    uint64_t *d_out = (uint64_t *)(d_buf + pyramid + list);

    const LaunchCfg cfg{s->stream, s->grid_cap};
    double total = 0.0;
    const char *step = "upload";
    hipError_t e = hipMemcpyAsync(d_draws, draws, list, hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) step = "chunk sums", e = launch_sample_chunk_sums(cfg, s->amps, s->f32, s->n, d_w);
    if (e == hipSuccess) step = "prefix", e = launch_sample_prefix(cfg, s->n, d_w, d_t);
    if (e == hipSuccess) step = "total", e = hipMemcpyAsync(&total, d_t + (g.groups - 1), 8, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    const bool drawable = total > 0.0 && std::isfinite(total); // a zero state (or one that holds no numbers) has no distribution
    if (e == hipSuccess && drawable) {
        step = "draws", e = launch_sample_draws(cfg, s->amps, s->f32, s->n, d_w, d_t, d_draws, shots, qs, d_out);
        if (e == hipSuccess) step = "download", e = hipMemcpyAsync(out, d_out, list, hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    }
    (void)hipFree(d_buf);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? QSIM_ERR_ALLOC : QSIM_ERR_DEVICE, "%s: %s: %s", who, step, hipGetErrorString(e));
    if (total_out) *total_out = total;
    if (!drawable) return fail(QSIM_ERR_ARG, "%s: the state's total probability is %g, nothing to draw from", who, total);
    return QSIM_OK;
}

extern "C" int qsim_sample_shots(qsim_state *s, const double *draws, long shots, const int *qubits, int num_qubits, uint64_t *out) {
    return sample_outcomes(s, "qsim_sample_shots", draws, shots, qubits, num_qubits, out, nullptr);
}
