// profile.cpp — the profiling events recorded around launches (LaunchScope, engine_state.h), the statistics and the launch log
// they resolve into, and the accessors of both.  Touches qsim_state's stats, events and launch_log only.
#include <algorithm>
#include <cstring>

#include "engine_state.h"

using namespace qsim;

// ---- profiling events ----------------------------------------------------------------------------------
hipEvent_t qsim::take_event(qsim_state *s) {
    if (!s->event_pool.empty()) {
        hipEvent_t e = s->event_pool.back();
        s->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

static int resolve_events(qsim_state *s) {
    if (s->events.empty()) return QSIM_OK;
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (auto &pe : s->events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pe.start, pe.stop) == hipSuccess) s->stats.k_ms[pe.kclass] += ms;
        if (s->launch_log.size() < (1u << 20)) s->launch_log.push_back({pe.kclass, pe.n_ops, pe.high_mask, (double)ms, pe.order_code, pe.visited, pe.read_share, std::move(pe.forms), std::move(pe.heads)});
        s->event_pool.push_back(pe.start);
        s->event_pool.push_back(pe.stop);
    }
    s->events.clear();
    return QSIM_OK;
}

extern "C" int qsim_get_stats(qsim_state *s, qsim_stats *out) {
    if (!s || !out) return fail(QSIM_ERR_ARG, "NULL argument");
    QSIM_TRY(resolve_events(s));
    *out = s->stats;
    return QSIM_OK;
}

extern "C" int qsim_reset_stats(qsim_state *s) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    QSIM_TRY(resolve_events(s));
    memset(&s->stats, 0, sizeof s->stats);
    s->launch_log.clear();
    return QSIM_OK;
}

// Record `index` of the launch log with every pending event resolved, or NULL and why in err.
static const LaunchRec *log_record(qsim_state *s, long index, int &err) {
    err = !s ? QSIM_ERR_ARG : resolve_events(s) ? QSIM_ERR_DEVICE : index < 0 || index >= (long)s->launch_log.size() ? QSIM_ERR_ARG : QSIM_OK;
    return err ? nullptr : &s->launch_log[index];
}

extern "C" int qsim_launch_log_order(qsim_state *s, long index, int *order, int *count) {
    int err = QSIM_ERR_ARG;
    const LaunchRec *rec = order && count ? log_record(s, index, err) : nullptr;
    if (!rec) return err;
    const LaunchRec &r = *rec;
    const int n = __builtin_popcountll(r.high_mask);
    for (int j = 0; j < n; j++) order[j] = (int)((r.order_code >> (5 * j)) & 31u);
    *count = r.kclass == QSIM_K_TILE ? n : 0;
    return QSIM_OK;
}

extern "C" int qsim_launch_log_visited(qsim_state *s, long index, double *visited) {
    int err = QSIM_ERR_ARG;
    const LaunchRec *rec = visited ? log_record(s, index, err) : nullptr;
    if (!rec) return err;
    *visited = rec->visited;
    return QSIM_OK;
}

extern "C" int qsim_launch_log_read_share(qsim_state *s, long index, double *read_share) {
    int err = QSIM_ERR_ARG;
    const LaunchRec *rec = read_share ? log_record(s, index, err) : nullptr;
    if (!rec) return err;
    *read_share = rec->read_share;
    return QSIM_OK;
}

extern "C" int qsim_launch_log_blocks(qsim_state *s, long index, uint8_t *codes, int cap, int *count) {
    int err = QSIM_ERR_ARG;
    const LaunchRec *rec = count ? log_record(s, index, err) : nullptr;
    if (!rec) return err;
    const std::vector<uint8_t> &f = rec->forms;
    *count = (int)f.size();
    for (int j = 0; codes && j < cap && j < (int)f.size(); j++) codes[j] = f[j];
    return QSIM_OK;
}

extern "C" int qsim_launch_log_block_flags(qsim_state *s, long index, uint8_t *codes, int cap, int *count) {
    int err = QSIM_ERR_ARG;
    const LaunchRec *rec = count ? log_record(s, index, err) : nullptr;
    if (!rec) return err;
    const std::vector<uint8_t> &f = rec->heads;
    *count = (int)(f.size() / kHeadBytes);
    for (size_t j = 0; codes && j < kHeadBytes * (size_t)std::max(cap, 0) && j < f.size(); j++) codes[j] = f[j];
    return QSIM_OK;
}

extern "C" long qsim_launch_log(qsim_state *s, long index, int *kclass, int *n_ops, uint64_t *high_mask, double *ms) {
    int err = QSIM_OK;
    const LaunchRec *r = log_record(s, index, err);
    if (!s || err == QSIM_ERR_DEVICE) return -1;
    if (r) {
        if (kclass) *kclass = r->kclass;
        if (n_ops) *n_ops = r->n_ops;
        if (high_mask) *high_mask = r->high_mask;
        if (ms) *ms = r->ms;
    }
    return (long)s->launch_log.size(); // whatever the index: that is how a caller learns the count
}
