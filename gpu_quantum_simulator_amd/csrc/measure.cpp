// measure.cpp — the host side of measure.hip: qsim_postselect (project onto a given outcome of k qubits and normalise), qsim_measure
// (the outcome drawn by ONE draw of sample.cpp's sampler, then the same two sweeps), qsim_collapse_plan (host only) and the sweep
// counter (measure.h has the rule).  A call joins the buffer, settles the state, runs the weight sweep, waits once for W,
// and runs the collapse sweep with f = 1 / sqrt(W) without waiting for it.  Nothing passes through the gate queue or the scheduler.
#include <atomic>
#include <cmath>

#include "engine_state.h"
#include "measure.h"
#include "subset_sweep.h" // qubit_list_mask, trips_at_cap

using namespace qsim;

namespace {

struct Outcome {
    uint64_t measured = 0, bits = 0; // the measured qubits, and the outcome deposited on them: bit j of the outcome is qubits[j]
};

bool outcome_masks(const int *qubits, int k, uint64_t outcome, int n, Outcome *out) {
    if (n < 0 || n > 40 || k < 0 || k > n || !qubit_list_mask(qubits, k, n, 0, &out->measured)) return false;
    if (k < 64 && (outcome >> k) != 0) return false;
    out->bits = 0;
    for (int j = 0; j < k; j++) out->bits |= ((outcome >> j) & 1ULL) << qubits[j];
    return true;
}

int refuse_list(const char *who, int n) {
    return fail(QSIM_ERR_ARG, "%s: 0 to %d distinct qubits inside the register of %d and an outcome below 2^k", who, n, n);
}

std::atomic<uint64_t> g_collapse_sweeps{0};

// The two sweeps on a settled state.  W == 0 or not finite: QSIM_ERR_ARG, the collapse is not launched and no bit has changed.
int collapse_onto(qsim_state *s, const char *who, const Outcome &o, double *weight) {
    QSIM_TRY(alloc_sweep_scratch(s));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    QSIM_TRY(launched("collapse weight sweep", launch_collapse_weight(cfg, s->amps, s->f32, s->n, o.measured, o.bits, sweep_partials(s), sweep_result_row(s))));
    double W = 0.0;
    QSIM_TRY(fetch_sweep_results(s, 1, &W)); // the call's one synchronisation
    *weight = W;
    if (!(W > 0.0) || !std::isfinite(W)) return fail(QSIM_ERR_ARG, "%s: outcome has probability zero (its weight is %g)", who, W);
    QSIM_TRY(launched("collapse sweep", launch_collapse(cfg, s->amps, s->f32, s->n, o.measured, o.bits, 1.0 / std::sqrt(W))));
    g_collapse_sweeps += 2;
    return QSIM_OK;
}

} // namespace

extern "C" uint64_t qsim_collapse_sweeps_launched(void) { return g_collapse_sweeps.load(); }

extern "C" int qsim_collapse_plan(const int *qubits, int k, uint64_t outcome, int num_q, int precision_bits, uint64_t *weight_units, uint64_t *collapse_units,
                                  long *weight_trips, long *collapse_trips) {
    const char *who = "qsim_collapse_plan";
    if (!weight_units || !collapse_units || !weight_trips || !collapse_trips) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    Outcome o;
    if (!outcome_masks(qubits, k, outcome, num_q, &o)) return refuse_list(who, num_q);
    const bool f32 = precision_bits == 32;
    *weight_units = collapse_weight_geom(o.measured, o.bits, f32, num_q).units;
    *collapse_units = collapse_geom(o.measured, o.bits, f32, num_q).units;
    const uint64_t per_trip = (uint64_t)kTPB * kCollapseUnitsPerTrip;
    *weight_trips = trips_at_cap(*weight_units, per_trip, kCollapseWeightGridCap);
    *collapse_trips = trips_at_cap(*collapse_units, per_trip, kCollapseGridCap);
    return QSIM_OK;
}

extern "C" int qsim_postselect(qsim_state *s, const int *qubits, int k, uint64_t outcome, double *weight) {
    const char *who = "qsim_postselect";
    if (!s || !weight) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    Outcome o;
    if (!outcome_masks(qubits, k, outcome, s->n, &o)) return refuse_list(who, s->n);
    if (qsim_holds_nothing(s)) return fail(QSIM_ERR_ARG, "%s: outcome has probability zero (the state holds nothing)", who);
    QSIM_TRY(await_buffer(s));
    QSIM_TRY(settle(s));
    return collapse_onto(s, who, o, weight);
}

extern "C" int qsim_measure(qsim_state *s, const int *qubits, int k, double draw, uint64_t *outcome, double *probability) {
    const char *who = "qsim_measure";
    if (!s || !outcome || !probability) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    Outcome o;
    if (!outcome_masks(qubits, k, 0, s->n, &o)) return refuse_list(who, s->n);
    if (!(draw >= 0.0 && draw <= 1.0)) return fail(QSIM_ERR_ARG, "%s: the draw is %g, not a number in [0, 1]", who, draw);
    if (qsim_holds_nothing(s)) return fail(QSIM_ERR_ARG, "%s: the state holds nothing, there is nothing to draw from", who);
    QSIM_TRY(await_buffer(s));
    QSIM_TRY(settle(s));
    // the sampler's own path: the pyramid, one draw, the outcome read off the drawn index (no qubits: the index itself, whose outcome
    // on no qubits is 0)
    uint64_t drawn = 0;
    double total = 0.0;
    QSIM_TRY(sample_outcomes(s, who, &draw, 1, qubits, k, &drawn, &total));
    if (k == 0) drawn = 0;
    if (!outcome_masks(qubits, k, drawn, s->n, &o)) return fail(QSIM_ERR_DEVICE, "%s: the sampler returned %llu on %d qubits", who, (unsigned long long)drawn, k);
    double W = 0.0;
    QSIM_TRY(collapse_onto(s, who, o, &W));
    *outcome = drawn;
    *probability = W / total;
    return QSIM_OK;
}
