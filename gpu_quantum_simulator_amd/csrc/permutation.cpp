// permutation.cpp — permutations of the basis states of up to ten target qubits under controls: the plan (the one place that decides
// the tile), the operand the kernel is handed, and the entry points.  The kernel is permutation.hip's; permutation.h has
// the tile rule they share.  The call settles the state, launches one in-place sweep of the control subspace on the state's stream
// and returns without waiting: the destination map travels through matrix.cpp's pinned staging ring to the state's sweep scratch,
// both stream-ordered.
#include <atomic>
#include <vector>

#include "engine_state.h"
#include "matrix.h" // kMatrixCoefDoubles: the size of a staging slot
#include "permutation.h"

using namespace qsim;

static_assert(((size_t)1 << perm_tile_bits(true)) * sizeof(uint16_t) <= kMatrixCoefDoubles * sizeof(double), "the largest map fits a staging slot");
static_assert(perm_tile_bits(true) <= 16 && perm_tile_bits(false) <= 16, "a tile-local index is a uint16");
static_assert(kPermMaxQubits + 2 <= perm_tile_bits(false), "ten high targets leave the tile two padding bits");

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
bool qsim::permutation_plan(const int *targets, int k, const int *controls, int num_controls, int n, bool f32, PermutationPlan *out) {
    uint64_t tmask, cmask;
    if (n < 0 || n > 40 || k > kPermMaxQubits) return false;
    if (!qubit_list_mask(targets, k, n, 0, &tmask) || !qubit_list_mask(controls, num_controls, n, tmask, &cmask)) return false;
    PermutationPlan p{};
    std::copy(targets, targets + k, p.targets);
    p.n = n, p.k = k, p.num_controls = num_controls, p.f32 = f32, p.controls = cmask;
    const int free_bits = n - num_controls; // the targets are among them
    p.tile_bits = free_bits < perm_tile_bits(f32) ? free_bits : perm_tile_bits(f32);
    p.path = p.tile_bits == perm_tile_bits(f32) ? 1 : 0;
    p.mask = pad_subset(tmask, cmask, p.tile_bits, n);
    p.tiles = 1ULL << (free_bits - p.tile_bits);
    p.units = (1ULL << free_bits) >> (f32 ? 1 : 0);
    if (p.units == 0) p.units = 1; // one active fp32 amplitude
    p.trips_at_cap = trips_at_cap(p.tiles, 1, kPermGridCap);
    *out = p;
    return true;
}

// ---- the operand ------------------------------------------------------------------------------------------------------------------
// perm: 2^k entries, each below 2^k and each once
static bool is_bijection(const uint32_t *perm, int k) {
    const uint32_t dim = 1u << k;
    std::vector<bool> seen(dim, false);
    for (uint32_t j = 0; j < dim; j++) {
        if (perm[j] >= dim || seen[perm[j]]) return false;
        seen[perm[j]] = true;
    }
    return true;
}

// where tile-local index u goes: its target bits through the caller's table (in the caller's order), its padding bits kept
static std::vector<uint16_t> local_map(const PermutationPlan &p, const uint32_t *perm) {
    const SubsetOrder order{p.mask, p.targets, p.k};
    const uint32_t all = (1u << p.tile_bits) - 1u, own = order.own(), pad = all & ~own;
    std::vector<uint16_t> map((size_t)all + 1);
    // u = a | b, a over the target bits and b over the padding bits (x -> (x - m) & m steps through the subsets of m and ends at 0):
    // the table is looked up once per a, 2^k times and not 2^B times — the call forms the map between two launches on the stream
    uint32_t a = 0;
    do {
        const uint32_t to = order.to_subset(perm[order.to_callers(a)]);
        uint32_t b = 0;
        do {
            map[a | b] = (uint16_t)(to | b);
            b = (b - pad) & pad;
        } while (b != 0);
        a = (a - own) & own;
    } while (a != 0);
    return map;
}

static int to_plan(const char *who, const uint32_t *perm, const int *targets, int k, const int *controls, int num_controls, int n, bool f32,
                   PermutationPlan *p) {
    if (!permutation_plan(targets, k, controls, num_controls, n, f32, p))
        return fail(QSIM_ERR_ARG, "%s: 0 to %d distinct target qubits and any number of distinct control qubits, disjoint, inside the register of %d", who,
                    kPermMaxQubits, n);
    if (perm && !is_bijection(perm, k)) return fail(QSIM_ERR_ARG, "%s: the table is not a bijection of [0, 2^%d)", who, k);
    return QSIM_OK;
}

extern "C" int qsim_apply_permutation_max_qubits(void) { return kPermMaxQubits; }

extern "C" int qsim_apply_permutation_plan(const int *targets, int k, const int *controls, int num_controls, int num_q, int precision_bits, int *path,
                                           int *tile_bits, uint64_t *tile_mask, uint64_t *tiles, uint64_t *units, long *trips_per_workgroup) {
    const char *who = "qsim_apply_permutation_plan";
    if (!path || !tile_bits || !tile_mask || !tiles || !units || !trips_per_workgroup) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    PermutationPlan p;
    QSIM_TRY(to_plan(who, nullptr, targets, k, controls, num_controls, num_q, precision_bits == 32, &p));
    *path = p.path, *tile_bits = p.tile_bits, *tile_mask = p.mask, *tiles = p.tiles, *units = p.units, *trips_per_workgroup = p.trips_at_cap;
    return QSIM_OK;
}

extern "C" int qsim_apply_permutation_operand(const uint32_t *perm, const int *targets, int k, const int *controls, int num_controls, int num_q,
                                              int precision_bits, uint16_t *map, int *entries) {
    const char *who = "qsim_apply_permutation_operand";
    if (!perm || !map || !entries) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    QSIM_TRY(check_register_args(who, num_q, precision_bits));
    PermutationPlan p;
    QSIM_TRY(to_plan(who, perm, targets, k, controls, num_controls, num_q, precision_bits == 32, &p));
    const std::vector<uint16_t> m = local_map(p, perm);
    std::copy(m.begin(), m.end(), map);
    *entries = (int)m.size();
    return QSIM_OK;
}

// ---- the call ---------------------------------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_permutation_sweeps{0};
extern "C" uint64_t qsim_permutation_sweeps_launched(void) { return g_permutation_sweeps.load(); }

extern "C" int qsim_apply_permutation(qsim_state *s, const uint32_t *perm, const int *targets, int k, const int *controls, int num_controls) {
    const char *who = "qsim_apply_permutation";
    if (!s || !perm) return fail(QSIM_ERR_ARG, "%s: NULL argument", who);
    PermutationPlan p;
    QSIM_TRY(to_plan(who, perm, targets, k, controls, num_controls, s->n, s->f32, &p));
    if (qsim_holds_nothing(s)) return QSIM_OK; // the zero vector stays the zero vector
    QSIM_TRY(await_buffer(s));
    QSIM_TRY(settle(s));
    const std::vector<uint16_t> map = local_map(p, perm);
    QSIM_TRY(stage_sweep_operand(s, map.data(), map.size() * sizeof(uint16_t)));
    const LaunchCfg cfg{s->stream, s->grid_cap};
    QSIM_TRY(launched("qsim_apply_permutation:", launch_permutation(cfg, s->amps, p, reinterpret_cast<const uint16_t *>(sweep_coef_staging(s)))));
    g_permutation_sweeps++;
    return QSIM_OK;
}
