// planning.h — what the three files of the planning step share beyond engine_state.h.  Who defines what:
//   wisdom.cpp      the process-wide tables (measured tile-bit orders, schedule hints, measured schedule choices), their locks and
//                   their epoch, all private to it; the lookups the engine uses (order_tile_bits, apply_sched_hint, have_sched_hints,
//                   wisdom_epoch: declared in engine_state.h), the entries the planning makes, and the file format
//                   (qsim_tune_table_*).  No HIP call.
//   planning.cpp    what needs a state: the schedule choice by the pass-time model (choose_schedule, qsim_choose_schedule*,
//                   qsim_support_after) and the timed planning on the device (qsim_tune_circuit*)
//   plan_probe.cpp  the device-free probes of a circuit's schedule (qsim_plan_circuit*, qsim_plan_passes, qsim_schedule_circuit*,
//                   qsim_tile_records).  No qsim_state, no HIP call.
#ifndef QSIM_PLANNING_H
#define QSIM_PLANNING_H

#include <atomic>

#include "engine_state.h"

namespace qsim {

// ---- wisdom.cpp ------------------------------------------------------------------------------------------------------------
// Scheduler variant per circuit, decided by the planning step: key -> the fields of SchedConfig that the variants differ in.
struct SchedHint { int commute; double cheap_margin; int lookahead; int cap; /* clusters per pass; 0: the configuration's own */ uint64_t seed; /* SchedConfig::seed */
                   int defer; /* SchedConfig::defer_flips (the engine still asks whether the flush at hand may: may_defer_flips) */
                   int support_weight; /* SchedConfig::support_weight */ };
struct RankedVariant { SchedHint hint; double cost; bool is_default; };
SchedConfig with_hint(SchedConfig v, const SchedHint &h);
// Files the choice under `key` (the default schedule is the absence of a hint; scfg says what the default is) and bumps the epoch
// if that changes how the circuit is scheduled.
void set_sched_hint(uint64_t key, const SchedHint &now, bool is_default, const SchedConfig &scfg);
// Circuits whose schedule was chosen by MEASUREMENT: the choice stands until the tables are cleared.
bool measured_choice(uint64_t key, RankedVariant &out);
void remember_measured_choice(uint64_t key, const RankedVariant &choice);
// The measured order of a tile pass's high bits: is there one for this bit set on this register (new_mask: the high bits outside
// the support when the pass starts), and "this is it" — g.high in the order to keep.  Entering bumps the epoch.
bool tile_order_known(const qsim_state *s, const TileGeom &g, uint64_t new_mask);
void enter_tile_order(const qsim_state *s, const TileGeom &g, uint64_t new_mask, float ms, float ms_ascending);
// Fisher-Yates over g.high, and the seed of the probe orders (QSIM_OPT_DEBUG_TILE_ORDER = k, qsim_tile_records' order_seed = k) for
// the pass-th tile pass, counted from 1.
void shuffle_high(TileGeom &g, uint64_t seed);
inline uint64_t probe_order_seed(uint64_t k, uint64_t pass) { return 0x9E3779B97F4A7C15ULL * (k + 1) + 0xD1B54A32D192ED03ULL * pass; }

// ---- planning.cpp ----------------------------------------------------------------------------------------------------------
// The candidates of the schedule choice and their prices by the pass-time model (the comment at the definition); no state, no HIP call.
size_t rank_schedules(const SchedConfig &scfg, const std::vector<QueuedGate> &q, bool f32, bool with_defer, const std::atomic<bool> *stop,
                      std::vector<SchedHint> &variants, std::vector<RankedVariant> *ranked);

// ---- plan_probe.cpp --------------------------------------------------------------------------------------------------------
// The circuit as the gate queue qsim_run_circuit would leave in a state (what the plan and schedule-hint keys are computed from).
std::vector<QueuedGate> queue_of(const qsim_circuit *c);
// The passes of these gates under this configuration, all at once.
std::vector<Pass> schedule(const SchedConfig &cfg, const std::vector<QueuedGate> &gates, uint64_t *gates_seen = nullptr, uint64_t *residual_flips = nullptr);

} // namespace qsim

#endif
