// state_algebra.cpp — the calls that take MORE than one state: copy, inner product and linear combination.  The
// kernels are combine.hip's and, for the inner product, expect.hip's paired sweep over two buffers; nothing here launches a kernel
// of its own.  Every entry point checks its arguments before anything is touched, settles the states involved, and orders the
// streams: states have streams of their own, so the work (on the destination's stream; qsim_inner: on a's) waits for an event
// recorded on every source's stream, and every source's stream waits for an event recorded behind the work — a gate queued on a
// source afterwards cannot overtake the read.
#include <cmath>

#include "engine_state.h"
#include "pauli_sweep.h"

using namespace qsim;

// `from`'s stream has reached this point before `to`'s stream goes on
static int stream_waits(qsim_state *to, qsim_state *from) {
    if (to == from || to->stream == from->stream) return QSIM_OK;
    hipEvent_t ev;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, from->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(to->stream, ev, 0);
    (void)hipEventDestroy(ev); // released once it has completed
    if (e != hipSuccess) return fail(QSIM_ERR_DEVICE, "ordering two states' streams failed: %s", hipGetErrorString(e));
    return QSIM_OK;
}

static int same_shape(const char *who, const qsim_state *a, const qsim_state *b) {
    if (a->n != b->n || a->f32 != b->f32 || a->device != b->device)
        return fail(QSIM_ERR_ARG, "%s: the states differ in qubit count, precision or device", who);
    return QSIM_OK;
}

// The destination of a pure write: queued gates and a pending |0...0> are dropped with what they would have produced, no zeros are
// written first, and the state is an ordinary dense one from here on.
static int settle_overwritten(qsim_state *dst) {
    QSIM_TRY(await_buffer(dst));
    dst->queue.clear();
    dst->zero_ket_pending = false;
    dst->partial = false;
    HIP_TRY(hipSetDevice(dst->device));
    return QSIM_OK;
}

extern "C" int qsim_copy_state(qsim_state *dst, qsim_state *src) {
    if (!dst || !src) return fail(QSIM_ERR_ARG, "qsim_copy_state: NULL state");
    if (dst == src) return fail(QSIM_ERR_ARG, "qsim_copy_state: the destination is the source");
    QSIM_TRY(same_shape("qsim_copy_state", dst, src));
    QSIM_TRY(settle(src));
    QSIM_TRY(settle_overwritten(dst));
    QSIM_TRY(stream_waits(dst, src));
    HIP_TRY(hipMemcpyAsync(dst->amps, src->amps, dst->amp_bytes() << dst->n, hipMemcpyDeviceToDevice, dst->stream));
    return stream_waits(src, dst);
}

extern "C" int qsim_inner(qsim_state *a, qsim_state *b, double *re, double *im) {
    if (!a || !b || !re || !im) return fail(QSIM_ERR_ARG, "qsim_inner: NULL argument");
    QSIM_TRY(same_shape("qsim_inner", a, b));
    QSIM_TRY(settle(b));
    QSIM_TRY(settle(a));
    QSIM_TRY(alloc_sweep_scratch(a));
    if (a != b) QSIM_TRY(stream_waits(a, b));
    // x == 0 over two buffers: every index, its partner the same index of the other state; slot 0 sums Re, slot 1 Im of
    // conj(partner) visited, so b is the visited buffer and a the partner: sum conj(a_i) b_i
    ExpectSweep sw{};
    sw.full = true;
    sw.count = 2;
    sw.im_mask = 0b10;
    const LaunchCfg cfg{a->stream, a->grid_cap};
    QSIM_TRY(launched("inner product", launch_expect(cfg, b->amps, a->amps, a->f32, a->n, sw, sweep_partials(a), sweep_result_row(a))));
    if (a != b) QSIM_TRY(stream_waits(b, a));
    double out[2];
    QSIM_TRY(fetch_sweep_results(a, 2, out));
    *re = out[0];
    *im = a == b ? 0.0 : out[1]; // Im conj(x) x is +-0 term by term
    return QSIM_OK;
}

extern "C" int qsim_combine(qsim_state *dst, const double d[2], qsim_state *p, const double a[2], qsim_state *q, const double b[2], double *norm2) {
    const char *who = "qsim_combine";
    if (!dst || !d || !p || !a || (q && !b)) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    if (dst == p || dst == q) return fail(QSIM_ERR_ARG, "%s: the destination is one of the sources", who);
    QSIM_TRY(same_shape(who, dst, p));
    if (q) QSIM_TRY(same_shape(who, dst, q));
    if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(a[0]) || !std::isfinite(a[1]) || (q && (!std::isfinite(b[0]) || !std::isfinite(b[1]))))
        return fail(QSIM_ERR_ARG, "%s: a non-finite coefficient", who);
    const bool load_dst = d[0] != 0.0 || d[1] != 0.0;
    QSIM_TRY(settle(p));
    if (q && q != p) QSIM_TRY(settle(q));
    QSIM_TRY(load_dst ? settle(dst) : settle_overwritten(dst));
    QSIM_TRY(alloc_sweep_scratch(dst));
    QSIM_TRY(stream_waits(dst, p));
    if (q && q != p) QSIM_TRY(stream_waits(dst, q));
    const LaunchCfg cfg{dst->stream, dst->grid_cap};
    QSIM_TRY(launched("combine", launch_combine(cfg, dst->amps, load_dst ? d : nullptr, p->amps, a, q ? q->amps : nullptr, b, dst->f32, dst->n,
                                                sweep_partials(dst), sweep_result_row(dst))));
    QSIM_TRY(stream_waits(p, dst));
    if (q && q != p) QSIM_TRY(stream_waits(q, dst));
    if (norm2) QSIM_TRY(fetch_sweep_results(dst, 1, norm2));
    return QSIM_OK;
}
