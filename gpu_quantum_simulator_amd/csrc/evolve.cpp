// evolve.cpp — the host side of evolve.hip: Pauli-string rotations exp(-i theta/2 P) applied to a state in the caller's order
// (DESIGN "Pauli rotations").  A term that is X or Y on a single qubit is a 2x2 for the gate queue; every other term goes to an
// in-place sweep, and consecutive sweep terms with one x mask share a sweep.  Like readout.cpp it opens with settle() and then
// only touches qsim_state's buffer and stream; unlike it, it writes the buffer.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "engine_state.h"

using namespace qsim;

// Terms per sweep: 32, the record count of k_pauli_rot; not backed by a measurement yet (DESIGN "Pauli rotations").
static constexpr int kPauliRotationsPerSweep = kMaxRotTermsPerSweep;
extern "C" int qsim_pauli_rotations_per_sweep(void) { return kPauliRotationsPerSweep; }

static std::atomic<uint64_t> g_sweeps_launched{0};
extern "C" uint64_t qsim_pauli_rotation_sweeps_launched(void) { return g_sweeps_launched.load(); }

long qsim::rotation_sweeps(long run_length) { return (run_length + kPauliRotationsPerSweep - 1) / kPauliRotationsPerSweep; }

static bool is_gate(uint64_t x, uint64_t z, uint64_t local_mask) {
    return __builtin_popcountll(x) == 1 && (z & ~x) == 0 && (x & local_mask) != 0;
}

std::vector<RotRoute> qsim::route_rotations(const uint64_t *X, const uint64_t *Z, long num, uint64_t local_mask) {
    std::vector<RotRoute> out;
    for (long t = 0; t < num;) {
        if (is_gate(X[t], Z[t], local_mask)) {
            out.push_back({t, 1, true});
            t++;
            continue;
        }
        long e = t + 1;
        while (e < num && X[e] == X[t] && !is_gate(X[e], Z[e], local_mask)) e++;
        out.push_back({t, e - t, false});
        t = e;
    }
    return out;
}

void qsim::pauli_rot_1q(bool y, double theta, double *U) {
    const double c = std::cos(0.5 * theta), sn = std::sin(0.5 * theta);
    const double ux[8] = {c, 0, 0, -sn, 0, -sn, c, 0}, uy[8] = {c, 0, -sn, 0, sn, 0, c, 0};
    std::copy(y ? uy : ux, (y ? uy : ux) + 8, U);
}

int qsim::pauli_rot_run(qsim_state *s, void *partner, uint64_t rank, uint64_t x, const uint64_t *Z, const double *thetas, long count) {
    if (!s || count < 0 || (count > 0 && (!Z || !thetas))) return fail(QSIM_ERR_ARG, "rotation: NULL argument or negative term count");
    const int m = s->n;
    const uint64_t mmask = index_mask(m);
    if (((x >> m) != 0) != (partner != nullptr)) return fail(QSIM_ERR_ARG, "rotation: a partner buffer goes with x on rank qubits, and only with it");
    if (count == 0 || (!partner && qsim_holds_nothing(s))) return QSIM_OK; // rotations map the zero vector to itself
    QSIM_TRY(settle(s));
    HIP_TRY(hipSetDevice(s->device)); // a cluster drives several devices from one thread, and settle() may have had nothing to do
    const LaunchCfg cfg{s->stream, s->grid_cap};
    for (long first = 0; first < count; first += kPauliRotationsPerSweep) {
        RotSweep sw{};
        sw.x = x & mmask;
        sw.full = partner != nullptr;
        sw.count = (int)std::min<long>(kPauliRotationsPerSweep, count - first);
        for (int k = 0; k < sw.count; k++) {
            const uint64_t z = Z[first + k];
            const double half = 0.5 * thetas[first + k], sn = std::sin(half);
            const int ny = __builtin_popcountll(x & z);
            // w = -i sin(theta/2) i^ny: -i sn, sn, i sn, -sn for ny = 0, 1, 2, 3 mod 4
            double v = (ny & 3) == 1 || (ny & 3) == 2 ? sn : -sn;
            if (__builtin_popcountll(rank & (z >> m)) & 1) v = -v; // Z on rank qubits: a sign per shard
            sw.z[k] = z & mmask;
            sw.c[k] = std::cos(half);
            sw.v[k] = v;
            if (ny & 1) sw.odd_mask |= 1u << k;
        }
        const hipError_t e = launch_pauli_rot(cfg, s->amps, partner ? partner : s->amps, s->f32, m, sw);
        if (e != hipSuccess) return fail(QSIM_ERR_DEVICE, "rotation sweep launch failed: %s", hipGetErrorString(e));
        g_sweeps_launched++;
    }
    return QSIM_OK;
}

extern "C" int qsim_pauli_rotation_plan(const uint64_t *x_masks, const uint64_t *z_masks, long num_terms, long *sweeps, long *queued_as_gates) {
    if (num_terms < 0) return fail(QSIM_ERR_ARG, "qsim_pauli_rotation_plan: negative term count");
    if (!sweeps || !queued_as_gates || (num_terms > 0 && (!x_masks || !z_masks))) return fail(QSIM_ERR_ARG, "qsim_pauli_rotation_plan: NULL argument");
    *sweeps = *queued_as_gates = 0;
    for (const RotRoute &r : route_rotations(x_masks, z_masks, num_terms, ~0ULL)) {
        if (r.gate) ++*queued_as_gates;
        else *sweeps += rotation_sweeps(r.count);
    }
    return QSIM_OK;
}

extern "C" int qsim_apply_pauli_rotations(qsim_state *s, const uint64_t *x_masks, const uint64_t *z_masks, const double *thetas, long num_terms) {
    if (!s) return fail(QSIM_ERR_ARG, "NULL state");
    if (num_terms < 0) return fail(QSIM_ERR_ARG, "qsim_apply_pauli_rotations: negative term count");
    if (num_terms > 0 && (!x_masks || !z_masks || !thetas)) return fail(QSIM_ERR_ARG, "qsim_apply_pauli_rotations: NULL argument");
    const uint64_t nmask = index_mask(s->n);
    for (long t = 0; t < num_terms; t++) {
        if ((x_masks[t] | z_masks[t]) & ~nmask)
            return fail(QSIM_ERR_ARG, "qsim_apply_pauli_rotations: term %ld names a qubit outside the %d-qubit register", t, s->n);
        if (!std::isfinite(thetas[t])) return fail(QSIM_ERR_ARG, "qsim_apply_pauli_rotations: term %ld has a non-finite angle", t);
    }
    for (const RotRoute &r : route_rotations(x_masks, z_masks, num_terms, nmask)) {
        if (r.gate) {
            double U[8];
            pauli_rot_1q((z_masks[r.first] & x_masks[r.first]) != 0, thetas[r.first], U);
            QSIM_TRY(qsim_apply_1q(s, U, __builtin_ctzll(x_masks[r.first])));
        } else {
            QSIM_TRY(pauli_rot_run(s, nullptr, 0, x_masks[r.first], z_masks + r.first, thetas + r.first, r.count));
        }
    }
    return QSIM_OK;
}
