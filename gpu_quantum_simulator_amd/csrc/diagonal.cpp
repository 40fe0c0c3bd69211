// diagonal.cpp — whole-register diagonal operators: the qsim_diagonal object (a real fp64 table d[0..2^n) on the device), the plan,
// the set-up calls that fill and inspect a table, the two sweeps over a state, exp(-i gamma D) and <D>, <D^2>, and
// dst = w D |state> (qsim_diagonal_apply_into).  The gradient through diagonal phases is pauli.cpp's, which owns the adjoint algorithm
// (DESIGN §7k); what it needs of a table is exported at the end.
// The kernels are diagonal.hip's; diagonal.h has the work item they share with this file.
//
// Ordering.  Calls take effect in the order issued without the caller synchronising anything.  A table has a stream of its own for
// the set-up calls (add_terms, write, read, extrema), and every set-up call has FINISHED on it when it returns, so a sweep issued
// afterwards on any state's stream sees the table as the call left it.  The other direction: a sweep records an event behind itself
// on the state's stream (one per stream that has read the table), and a set-up call that modifies the table waits for all of them
// first.  The set-up calls block the host; the sweeps never do.  A table that is adopted (qsim_diagonal_create_external) is the
// caller's to keep in order with the caller's own work on it.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "diagonal.h"
#include "engine_state.h"
#include "subset_sweep.h" // trips_at_cap

using namespace qsim;

struct qsim_diagonal {
    int n = 0, device = 0;
    double *table = nullptr;   // 2^n doubles
    bool owns = false;
    hipStream_t stream = nullptr; // the set-up calls'
    double *d_scratch = nullptr;  // kDiagScratchDoubles: the extrema reduction
    struct Reader { hipStream_t stream; hipEvent_t done; bool pending; };
    std::vector<Reader> readers;  // the streams whose sweeps have read the table, and the event behind the last one of each
};

// The tables alive, so that a state that goes can tell them (forget_diagonal_reads): a table may outlive the states that swept it.
static std::mutex g_live_mutex;
static std::vector<qsim_diagonal *> g_live;

static int use_device(const char *who, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(QSIM_ERR_DEVICE, "%s: no HIP device available (libqsim has no CPU fallback)", who);
    if (device < 0 || device >= ndev) return fail(QSIM_ERR_ARG, "%s: device %d out of range (%d present)", who, device, ndev);
    HIP_TRY(hipSetDevice(device));
    return QSIM_OK;
}

// ---- creation and destruction -----------------------------------------------------------------------------------------------------
static int make_diagonal(const char *who, qsim_diagonal **out, int num_q, int device, void *ext) {
    if (!out) return fail(QSIM_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (num_q < 0 || num_q > 40) return fail(QSIM_ERR_ARG, "%s: a table over %d qubits", who, num_q);
    if (ext && num_q > 0 && ((uintptr_t)ext & 15u)) return fail(QSIM_ERR_ARG, "%s: the buffer is not aligned to 16 bytes", who);
    QSIM_TRY(use_device(who, device));
    qsim_diagonal *d = new qsim_diagonal();
    d->n = num_q, d->device = device;
    const size_t bytes = sizeof(double) << num_q;
    hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&d->d_scratch, kDiagScratchDoubles * sizeof(double));
    if (e == hipSuccess) {
        if (ext) d->table = (double *)ext;
        else {
            e = hipMalloc((void **)&d->table, bytes);
            d->owns = e == hipSuccess;
            if (e == hipSuccess) e = hipMemsetAsync(d->table, 0, bytes, d->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        const int code = fail(e == hipErrorOutOfMemory ? QSIM_ERR_ALLOC : QSIM_ERR_DEVICE, "%s: %s (the table needs %zu bytes)", who, hipGetErrorString(e), bytes);
        qsim_diagonal_destroy(d);
        return code;
    }
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_live.push_back(d);
    }
    *out = d;
    return QSIM_OK;
}

extern "C" int qsim_diagonal_create(qsim_diagonal **out, int num_q, int device) { return make_diagonal("qsim_diagonal_create", out, num_q, device, nullptr); }
extern "C" int qsim_diagonal_create_external(qsim_diagonal **out, int num_q, int device, void *device_doubles) {
    if (!device_doubles) return fail(QSIM_ERR_ARG, "qsim_diagonal_create_external: device_doubles is NULL");
    return make_diagonal("qsim_diagonal_create_external", out, num_q, device, device_doubles);
}

// every sweep that reads the table has run
static hipError_t wait_for_readers(qsim_diagonal *d) {
    for (auto &r : d->readers)
        if (r.pending) {
            const hipError_t e = hipEventSynchronize(r.done);
            if (e != hipSuccess) return e;
            r.pending = false;
        }
    return hipSuccess;
}

extern "C" void qsim_diagonal_destroy(qsim_diagonal *d) {
    if (!d) return;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_live.erase(std::remove(g_live.begin(), g_live.end(), d), g_live.end());
    }
    (void)hipSetDevice(d->device);
    (void)wait_for_readers(d);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    for (auto &r : d->readers) (void)hipEventDestroy(r.done);
    if (d->owns && d->table) (void)hipFree(d->table);
    if (d->d_scratch) (void)hipFree(d->d_scratch);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

extern "C" int qsim_diagonal_num_qubits(const qsim_diagonal *d) { return d ? d->n : -1; }
extern "C" void *qsim_diagonal_device_ptr(qsim_diagonal *d) { return d ? d->table : nullptr; }

// ---- the set-up calls -------------------------------------------------------------------------------------------------------------
// What every set-up call opens with: the table's device current, and every sweep that reads the table finished.
static int begin_setup(const char *who, qsim_diagonal *d) {
    if (!d) return fail(QSIM_ERR_ARG, "%s: NULL table", who);
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(wait_for_readers(d));
    return QSIM_OK;
}

extern "C" int qsim_diagonal_add_terms(qsim_diagonal *d, const uint64_t *z_masks, const double *coeffs, long num_terms) {
    const char *who = "qsim_diagonal_add_terms";
    if (!d) return fail(QSIM_ERR_ARG, "%s: NULL table", who);
    if (num_terms < 0) return fail(QSIM_ERR_ARG, "%s: negative term count", who);
    if (num_terms > 0 && (!z_masks || !coeffs)) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    for (long t = 0; t < num_terms; t++)
        if (z_masks[t] & ~index_mask(d->n)) return fail(QSIM_ERR_ARG, "%s: term %ld names a qubit outside the %d-qubit register", who, t, d->n);
    if (num_terms == 0) return QSIM_OK;
    QSIM_TRY(begin_setup(who, d));
    for (long first = 0; first < num_terms; first += kDiagTermsPerRecord) { // records in the caller's order, one launch each
        DiagTerms rec{};
        rec.count = (int32_t)std::min<long>(kDiagTermsPerRecord, num_terms - first);
        std::memcpy(rec.z, z_masks + first, (size_t)rec.count * sizeof(uint64_t));
        std::memcpy(rec.c, coeffs + first, (size_t)rec.count * sizeof(double));
        QSIM_TRY(launched("qsim_diagonal_add_terms:", launch_diag_add_terms(d->stream, d->table, d->n, rec)));
    }
    HIP_TRY(hipStreamSynchronize(d->stream));
    return QSIM_OK;
}

static int check_range(const char *who, const qsim_diagonal *d, uint64_t first, uint64_t count, const void *host) {
    if (!d) return fail(QSIM_ERR_ARG, "%s: NULL table", who);
    const uint64_t N = 1ULL << d->n;
    if (first > N || count > N - first) return fail(QSIM_ERR_ARG, "%s: entries [%llu, %llu + %llu) outside the table of 2^%d", who,
                                                     (unsigned long long)first, (unsigned long long)first, (unsigned long long)count, d->n);
    if (count > 0 && !host) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    return QSIM_OK;
}

extern "C" int qsim_diagonal_write(qsim_diagonal *d, uint64_t first, uint64_t count, const double *host) {
    const char *who = "qsim_diagonal_write";
    QSIM_TRY(check_range(who, d, first, count, host));
    if (count == 0) return QSIM_OK;
    QSIM_TRY(begin_setup(who, d));
    HIP_TRY(hipMemcpyAsync(d->table + first, host, count * sizeof(double), hipMemcpyHostToDevice, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return QSIM_OK;
}

extern "C" int qsim_diagonal_read(qsim_diagonal *d, uint64_t first, uint64_t count, double *host) {
    const char *who = "qsim_diagonal_read";
    QSIM_TRY(check_range(who, d, first, count, host));
    if (count == 0) return QSIM_OK;
    QSIM_TRY(begin_setup(who, d));
    HIP_TRY(hipMemcpyAsync(host, d->table + first, count * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return QSIM_OK;
}

extern "C" int qsim_diagonal_extrema(qsim_diagonal *d, double *min, uint64_t *argmin, double *max, uint64_t *argmax) {
    const char *who = "qsim_diagonal_extrema";
    if (!d || !min || !argmin || !max || !argmax) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(begin_setup(who, d));
    QSIM_TRY(launched("qsim_diagonal_extrema:", launch_diag_extrema(d->stream, d->table, d->n, d->d_scratch)));
    double row[kDiagExtremaRowDoubles];
    HIP_TRY(hipMemcpyAsync(row, d->d_scratch + (size_t)kDiagExtremaGrid * kDiagExtremaRowDoubles, sizeof(row), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    *min = row[0], *max = row[2];
    std::memcpy(argmin, &row[1], sizeof(uint64_t));
    std::memcpy(argmax, &row[3], sizeof(uint64_t));
    return QSIM_OK;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_diagonal_sweeps{0};
extern "C" uint64_t qsim_diagonal_sweeps_launched(void) { return g_diagonal_sweeps.load(); }

extern "C" int qsim_diagonal_plan(int num_q, int precision_bits, uint64_t *items, int *items_per_trip_phase, int *items_per_trip_expect,
                                  long *trips_at_cap_phase, long *trips_at_cap_expect) {
    const char *who = "qsim_diagonal_plan";
    if (!items || !items_per_trip_phase || !items_per_trip_expect || !trips_at_cap_phase || !trips_at_cap_expect) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    const DiagGeom g = diag_geom(num_q);
    const int per_trip = diag_items_per_trip(precision_bits == 32);
    *items = g.items;
    *items_per_trip_phase = *items_per_trip_expect = per_trip;
    const uint64_t blocks = (g.items + kTPB - 1) / kTPB; // items of kTPB threads
    const bool plain = g.items < (uint64_t)kDiagWave;    // one workgroup, one thread per amplitude
    *trips_at_cap_phase = plain ? 1 : trips_at_cap(blocks, (uint64_t)per_trip, kDiagPhaseGrid);
    *trips_at_cap_expect = plain ? 1 : trips_at_cap(blocks, (uint64_t)per_trip, kExpectGrid);
    return QSIM_OK;
}

// ---- the two sweeps over a state --------------------------------------------------------------------------------------------------
int qsim::check_diag_pair(const char *who, const qsim_state *s, const qsim_diagonal *d) {
    if (!s || !d) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    if (d->n != s->n) return fail(QSIM_ERR_ARG, "%s: a table over %d qubits on a state of %d", who, d->n, s->n);
    if (d->device != s->device) return fail(QSIM_ERR_ARG, "%s: the table lives on device %d, the state on device %d", who, d->device, s->device);
    return QSIM_OK;
}

// the event behind the sweep just launched on the state's stream: what a later modification of the table waits for
int qsim::mark_read(const qsim_state *s, const qsim_diagonal *cd) {
    qsim_diagonal *d = const_cast<qsim_diagonal *>(cd); // the bookkeeping is not the table
    qsim_diagonal::Reader *r = nullptr;
    for (auto &have : d->readers)
        if (have.stream == s->stream) r = &have;
    if (!r) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        d->readers.push_back({s->stream, ev, false});
        r = &d->readers.back();
    }
    HIP_TRY(hipEventRecord(r->done, s->stream));
    r->pending = true;
    return QSIM_OK;
}

// The state's stream has been waited for and is about to be destroyed: its sweeps have read what they read, and their events, last
// recorded on that stream, are not to be waited for any more (engine_state.h).
void qsim::forget_diagonal_reads(const qsim_state *s) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    for (qsim_diagonal *d : g_live)
        for (auto &r : d->readers)
            if (r.stream == s->stream) r.pending = false;
}

extern "C" int qsim_apply_diagonal_phase(qsim_state *s, const qsim_diagonal *d, double gamma) {
    const char *who = "qsim_apply_diagonal_phase";
    QSIM_TRY(check_diag_pair(who, s, d));
    if (!std::isfinite(gamma)) return fail(QSIM_ERR_ARG, "%s: a non-finite gamma", who);
    if (qsim_holds_nothing(s)) return QSIM_OK; // the zero vector stays the zero vector
    QSIM_TRY(await_buffer(s));
    QSIM_TRY(settle(s));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    QSIM_TRY(launched("qsim_apply_diagonal_phase:", launch_diag_phase(cfg, s->amps, s->f32, s->n, d->table, gamma / M_PI)));
    g_diagonal_sweeps++;
    return mark_read(s, d);
}

extern "C" int qsim_expect_diagonal(qsim_state *s, const qsim_diagonal *d, double out[2]) {
    const char *who = "qsim_expect_diagonal";
    QSIM_TRY(check_diag_pair(who, s, d));
    if (!out) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    out[0] = out[1] = 0.0;
    if (qsim_holds_nothing(s)) return QSIM_OK; // zeros, no sweep
    QSIM_TRY(await_buffer(s));
    QSIM_TRY(settle(s));
    QSIM_TRY(alloc_sweep_scratch(s));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    QSIM_TRY(launched("qsim_expect_diagonal:", launch_diag_expect(cfg, s->amps, s->f32, s->n, d->table, sweep_partials(s), sweep_result_row(s))));
    g_diagonal_sweeps++;
    QSIM_TRY(mark_read(s, d));
    return fetch_sweep_results(s, 2, out);
}

// ---- what pauli.cpp's gradient needs of a table (diagonal.h) ------------------------------------------------------------------------
const double *qsim::diag_table(const qsim_diagonal *d) { return d->table; }
void qsim::count_diagonal_sweep() { g_diagonal_sweeps++; }

// dst (= | +=) weight D |state>, out of place (k_diag_apply): the diagonal part of lambda = H psi on its own, as qsim_pauli_sum_into
// is the Pauli part
extern "C" int qsim_diagonal_apply_into(qsim_state *s, const qsim_diagonal *d, double weight, void *dst_device, int accumulate) {
    const char *who = "qsim_diagonal_apply_into";
    QSIM_TRY(check_diag_pair(who, s, d));
    if (!std::isfinite(weight)) return fail(QSIM_ERR_ARG, "%s: a non-finite weight", who);
    QSIM_TRY(await_buffer(s));
    if (!dst_device || dst_device == s->amps || dst_device == s->spare)
        return fail(QSIM_ERR_ARG, "%s: the destination is NULL or one of the state's own buffers", who);
    QSIM_TRY(settle(s));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    QSIM_TRY(launched("qsim_diagonal_apply_into:", launch_diag_apply(cfg, s->amps, dst_device, s->f32, s->n, d->table, weight, accumulate != 0)));
    g_diagonal_sweeps++;
    return mark_read(s, d);
}
